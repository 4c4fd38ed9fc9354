"""GPU tests of csrc/dtw.hip (dsp_dtw_pairwise, dsp_dtw_knn) and the Python surface on it.
Everything is compared with the numpy restatements of tests/dtw_reference.py on the raw bits:
the distance is defined bit for bit, so there is no tolerance and no row is left out."""
import functools
import wave

import numpy as np
import pytest

import dtw_reference as R

pytestmark = pytest.mark.gpu

CANARY = 64  # float64 / int32 elements after each buffer


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def _dev(x, dtype, fill):
    """x flat on the device followed by CANARY elements of ``fill``; (whole buffer, view of x)."""
    import torch
    x = np.ascontiguousarray(x)
    buf = torch.full((x.size + CANARY,), fill, dtype=dtype, device="cuda")
    buf[:x.size] = torch.as_tensor(x.reshape(-1)).to("cuda", dtype)
    return buf, buf[:x.size].view(x.shape)


def _tail_ok(buf, fill):
    import torch
    t = buf[-CANARY:]
    return bool(torch.isnan(t).all()) if fill != fill else bool((t == fill).all())


def pairwise_raw(a, la, b, lb, window):
    """dsp_dtw_pairwise through the bare C ABI.  NaN canaries follow both sequence buffers (a read
    past the last row would poison a result) and -7.0 follows dist (a write past it shows)."""
    import torch
    from src import _hip
    lib = _hip.lib()
    (Nq, Tq, F), (Nr, Tr, _) = a.shape, b.shape
    nan = float("nan")
    ba, ta = _dev(a, torch.float64, nan)
    bb, tb = _dev(b, torch.float64, nan)
    bla, tla = _dev(np.asarray(la, np.int32), torch.int32, 10 ** 6)
    blb, tlb = _dev(np.asarray(lb, np.int32), torch.int32, 10 ** 6)
    bd, td = _dev(np.full((Nq, Nr), -7.0), torch.float64, -7.0)
    nbytes = lib.dsp_dtw_workspace_bytes(Nr, Nq, Tr, Tq, F, 1)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.dsp_dtw_pairwise(_hip.ptr(ta), _hip.ptr(tla), Nq, Tq, _hip.ptr(tb), _hip.ptr(tlb), Nr, Tr, F, window,
                              _hip.ptr(td), _hip.ptr(ws), nbytes, _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    assert _tail_ok(bd, -7.0) and _tail_ok(ba, nan) and _tail_ok(bb, nan)
    return td.cpu().numpy()


def knn_raw(ref, lr, labels, q, lq, k, window=-1, self_offset=-1, with_pred=True):
    """dsp_dtw_knn through the bare C ABI -> (idx, dist, pred or None); canaries after idx / dist / pred."""
    import torch
    from src import _hip
    lib = _hip.lib()
    (Nr, Tr, F), (Nq, Tq, _) = ref.shape, q.shape
    tr = torch.as_tensor(np.ascontiguousarray(ref)).to("cuda", torch.float64)
    tq = torch.as_tensor(np.ascontiguousarray(q)).to("cuda", torch.float64)
    tlr = torch.as_tensor(np.asarray(lr, np.int32)).cuda()
    tlq = torch.as_tensor(np.asarray(lq, np.int32)).cuda()
    tl = torch.as_tensor(np.asarray(labels, np.int32)).cuda() if labels is not None else None
    bi, ti = _dev(np.full((Nq, k), -9, np.int32), torch.int32, -9)
    bd, td = _dev(np.full((Nq, k), -7.0), torch.float64, -7.0)
    bp, tp = _dev(np.full(Nq, -9, np.int32), torch.int32, -9)
    nbytes = lib.dsp_dtw_workspace_bytes(Nr, Nq, Tr, Tq, F, k)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.dsp_dtw_knn(_hip.ptr(tr), _hip.ptr(tlr), _hip.ptr(tl), Nr, Tr, _hip.ptr(tq), _hip.ptr(tlq), Nq, Tq, F,
                         window, k, self_offset, 0, _hip.ptr(ti), _hip.ptr(td), _hip.ptr(tp) if with_pred else None,
                         _hip.ptr(ws), nbytes, _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    assert _tail_ok(bi, -9) and _tail_ok(bd, -7.0) and _tail_ok(bp, -9)
    pred = tp.cpu().numpy()
    if not with_pred or labels is None:
        assert (pred == -9).all()  # the vote was skipped: pred untouched
        pred = None
    return ti.cpu().numpy(), td.cpu().numpy(), pred


def check_knn(got, want):
    (gi, gd, gp), (wi, wd, wp) = got, want
    assert np.array_equal(gi, wi)
    assert np.array_equal(bits(gd), bits(wd))
    assert (gp is None and wp is None) or np.array_equal(gp, wp)


table_case = R.table_case


@functools.lru_cache(maxsize=None)
def table_reference(F, window):
    return R.dtw_pairwise(*table_case(F), window)


@pytest.mark.parametrize("window", R.TABLE_WINDOWS)
@pytest.mark.parametrize("F", R.TABLE_F)
def test_pairwise_table(F, window):
    """19 x 37 pairs (no multiple of a tile or a wave) at T = 70: one, two and three strips, lengths
    1, 2, 31, 32, 33, 63, 64, 65, 70 on both sides and random ones, so n > m and n < m in every wave."""
    a, la, b, lb = table_case(F)
    want = table_reference(F, window)
    got = pairwise_raw(a, la, b, lb, window)
    assert np.isfinite(want).all()
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]


def test_pairwise_longest_sequences():
    """T = 1024 with lengths 1, 1023 and 1024 on either side (Nq = 2, Nr = 3 and the transposed call),
    against the wavefront restatement (held to the other two in tests/test_dtw_host.py)."""
    rng = np.random.default_rng(11)
    a, b = rng.normal(0, 1, (2, 1024, 2)), rng.normal(0, 1, (3, 1024, 2))
    la, lb = np.array([1024, 1], np.int32), np.array([1, 1023, 1024], np.int32)
    for window in (-1, 100):
        want = np.array([[R.dtw_wavefront(a[q, :la[q]], b[r, :lb[r]], window) for r in range(3)] for q in range(2)])
        assert np.array_equal(bits(pairwise_raw(a, la, b, lb, window)), bits(want))
        assert np.array_equal(bits(pairwise_raw(b, lb, a, la, window)), bits(want.T))


def test_pairwise_many_strips():
    """Random reference lengths up to 300 (ten strips, two tiles) at F = 5: strips and rows that a
    band makes inadmissible for a whole wave are skipped between strips that are not."""
    rng = np.random.default_rng(5)
    a, b = rng.normal(0, 1, (3, 300, 5)), rng.normal(0, 1, (70, 300, 5))
    la, lb = np.array([300, 97, 33], np.int32), rng.integers(1, 301, 70).astype(np.int32)
    for window in (-1, 7):
        want = np.array([[R.dtw_wavefront(a[q, :la[q]], b[r, :lb[r]], window) for r in range(70)] for q in range(3)])
        assert np.array_equal(bits(pairwise_raw(a, la, b, lb, window)), bits(want))


def test_invalid_lengths_give_inf_and_nothing_is_touched():
    """Lengths 0, -1 and T + 1 on both sides: +inf rows and columns, every other entry the
    reference's.  The padding of every row and the canaries after the last rows are NaN: nothing
    outside a sequence's own frames reaches a result, and nothing after dist is written (pairwise_raw)."""
    a, la, b, lb = (x.copy() for x in table_case(2))
    la[[2, 7, 11]] = [0, -1, 71]
    lb[[0, 20, 36]] = [71, 0, -1]
    for x, n in ((a, la), (b, lb)):
        for i in range(len(x)):
            if 1 <= n[i] <= 70:
                x[i, n[i]:] = np.nan
    for window in (-1, 3):
        got = pairwise_raw(a, la, b, lb, window)
        want = R.dtw_pairwise(np.nan_to_num(a), la, np.nan_to_num(b), lb, window)
        assert np.isinf(want[[2, 7, 11]]).all() and np.isinf(want[:, [0, 20, 36]]).all()
        assert np.isfinite(np.delete(np.delete(want, [2, 7, 11], 0), [0, 20, 36], 1)).all()
        assert np.array_equal(bits(got), bits(want))


def test_position_independence():
    """One pair at several (q, r) positions -- other lanes, other tiles, other waves' loop bounds --
    and alone (Nq = Nr = 1): equal bits; the dist of dsp_dtw_knn is dsp_dtw_pairwise's."""
    rng = np.random.default_rng(21)
    x, y = rng.normal(0, 1, (45, 3)), rng.normal(0, 1, (70, 3))
    for window in (-1, 5):
        alone = pairwise_raw(x[None], [45], y[None], [70], window)
        assert bits(alone)[0, 0] == bits(R.dtw_wavefront(x, y, window))
        a, la, b, lb = R.case(19, 133, 70, 3, seed=77)
        qpos, rpos = [0, 5, 18], [0, 36, 63, 64, 100, 132]
        for q in qpos:
            a[q], la[q] = 0.0, 45
            a[q, :45] = x
        for r in rpos:
            b[r], lb[r] = 0.0, 70
            b[r, :70] = y
        d = pairwise_raw(a, la, b, lb, window)
        assert (bits(d[np.ix_(qpos, rpos)]) == bits(alone)[0, 0]).all()
        idx, dist, _ = knn_raw(b, lb, None, a, la, 32, window)
        want = R.knn_from_dist(d, 32)
        assert np.array_equal(idx, want[0]) and np.array_equal(bits(dist), bits(want[1]))


@functools.lru_cache(maxsize=None)
def knn_case():
    """40 references at T = 40, F = 2: rows 0..5 are copies of one sequence (labels 3, 1, 2, 1, 3, 0),
    rows 10, 20 and 30 copies of another, the rest random; 9 queries, the first two those sequences."""
    rng = np.random.default_rng(31)
    ref, lr = R.case(9, 40, 40, 2, seed=32)[2:]
    s0, s1 = rng.normal(0, 1, (17, 2)), rng.normal(0, 1, (33, 2))
    for r in range(6):
        ref[r], lr[r] = 0.0, 17
        ref[r, :17] = s0
    for r in (10, 20, 30):
        ref[r], lr[r] = 0.0, 33
        ref[r, :33] = s1
    labels = rng.integers(0, 4, 40).astype(np.int32)
    labels[:6] = [3, 1, 2, 1, 3, 0]
    q, lq = R.case(9, 40, 40, 2, seed=33)[:2]
    q[0], lq[0] = 0.0, 17
    q[0, :17] = s0
    q[1], lq[1] = 0.0, 33
    q[1, :33] = s1
    return ref, lr, labels, q, lq, R.dtw_pairwise(q, lq, ref, lr, -1)


@pytest.mark.parametrize("k", [1, 3, 32])
def test_knn_rules(k):
    """Ascending distance, exact ties by the smaller index (the copies), the vote's tie to the smallest
    label, a NULL pred and NULL labels."""
    ref, lr, labels, q, lq, d = knn_case()
    want = R.knn_from_dist(d, k, labels)
    got = knn_raw(ref, lr, labels, q, lq, k)
    check_knn(got, want)
    assert got[0][0, :min(k, 6)].tolist() == [0, 1, 2, 3, 4, 5][:k] and (got[1][0, :min(k, 6)] == 0.0).all()
    assert got[0][1, :min(k, 3)].tolist() == [10, 20, 30][:k]
    assert got[2][0] == {1: 3, 3: 1, 32: want[2][0]}[k]  # k = 3: labels 3, 1, 2 tie -> 1
    check_knn(knn_raw(ref, lr, labels, q, lq, k, with_pred=False), (want[0], want[1], None))
    check_knn(knn_raw(ref, lr, None, q, lq, k), (want[0], want[1], None))


def test_knn_k_equals_nr_self_offset_and_too_few_candidates():
    ref, lr, labels, q, lq, d = knn_case()
    # k = Nr: every reference, in order
    sub = slice(0, 20)
    check_knn(knn_raw(ref[sub], lr[sub], labels[sub], q, lq, 20), R.knn_from_dist(d[:, sub], 20, labels[sub]))
    # a self-query: row self_offset + q is excluded (the copies of row 0 remain at distance 0)
    ds = R.dtw_pairwise(ref[3:12], lr[3:12], ref, lr, 2)
    got = knn_raw(ref, lr, labels, ref[3:12], lr[3:12], 3, window=2, self_offset=3)
    check_knn(got, R.knn_from_dist(ds, 3, labels, self_offset=3))
    assert got[0][0].tolist() == [0, 1, 2] and all(3 + i not in got[0][i] for i in range(9))
    # fewer than k references at a finite distance: idx -1, dist +inf; none at all: pred -1
    lr2 = lr.copy()
    lr2[2:] = 0
    want = R.knn_from_dist(R.dtw_pairwise(q, lq, ref, lr2, -1), 3, labels)
    got = knn_raw(ref, lr2, labels, q, lq, 3)
    check_knn(got, want)
    assert (got[0][:, 2] == -1).all() and np.isinf(got[1][:, 2]).all() and (got[0][:, :2] == [0, 1]).all()
    lq2 = lq.copy()
    lq2[4] = 41
    got = knn_raw(ref, lr, labels, q, lq2, 3)
    assert got[0][4].tolist() == [-1, -1, -1] and np.isinf(got[1][4]).all() and got[2][4] == -1
    check_knn(got, R.knn_from_dist(R.dtw_pairwise(q, lq2, ref, lr, -1), 3, labels))


def test_knn_query_chunks():
    """dsp_dtw_knn works through the queries in chunks of at most 1024 (csrc/dtw.hip DTW_QCHUNK):
    1024 + 7 queries reach the chunk size at test size, so two chunks run -- the second with another
    query offset in idx / dist / pred and in the self exclusion -- with no diagnostic build."""
    rng = np.random.default_rng(41)
    Nq, Nr, T = 1031, 5, 3
    q, ref = rng.normal(0, 1, (Nq, T, 1)), rng.normal(0, 1, (Nr, T, 1))
    lq, lr = rng.integers(1, T + 1, Nq).astype(np.int32), rng.integers(1, T + 1, Nr).astype(np.int32)
    labels = np.array([2, 0, 1, 0, 2], np.int32)
    d = R.dtw_pairwise(q, lq, ref, lr, -1)
    check_knn(knn_raw(ref, lr, labels, q, lq, 2), R.knn_from_dist(d, 2, labels))
    got = knn_raw(ref, lr, labels, q, lq, 2, self_offset=0)  # rows 0..4 exclude themselves, in chunk 0 only
    check_knn(got, R.knn_from_dist(d, 2, labels, self_offset=0))


@functools.lru_cache(maxsize=None)
def extracted():
    """60 synthetic clips through the fused kernel with return_sequences: (list of [n_i, 3] float64, labels)."""
    import torch
    from src.pipeline import FeatureExtractor
    from src.synth import make_batch
    pcm, y = make_batch(60, with_labels=True)
    out = FeatureExtractor(1102, 441, "hamming", True, return_sequences=True)(torch.as_tensor(pcm, device="cuda"))
    seq, n = out["seq"].cpu().numpy(), out["n_frames"].cpu().numpy()
    assert ((out["status"].cpu().numpy() & 0xFF) == 0).all() and n.min() >= 1 and n.max() <= seq.shape[1]
    assert seq.dtype == np.float32
    return [seq[i, :n[i]].astype(np.float64) for i in range(60)], y


def test_sequence_classifier_on_extracted_features():
    from src.models import SequenceClassifier
    seqs, y = extracted()
    tr, te, ytr = seqs[:45], seqs[45:], y[:45]
    clf = SequenceClassifier(n_neighbors=3).fit(tr, ytr)
    frames = np.concatenate(tr)
    mean, std = frames.mean(axis=0), frames.std(axis=0)
    std = np.where(std == 0, 1.0, std)
    a, la = R.pad([(s - mean) / std for s in te])
    b, lb = R.pad([(s - mean) / std for s in tr])
    classes, codes = np.unique(ytr, return_inverse=True)
    idx, dist, pred = R.knn_from_dist(R.dtw_pairwise(a, la, b, lb, -1), 3, codes)
    gd, gi = clf.kneighbors(te)
    labels = clf.predict(te)
    assert np.array_equal(gi, idx.astype(np.int64)) and np.array_equal(bits(gd), bits(dist))
    assert np.array_equal(labels, classes[pred])
    # padded + lengths input: the same answers, whatever the padding holds and however wide it is
    pte, nte = R.pad(te, T=max(len(s) for s in seqs) + 3)
    pte[np.arange(pte.shape[1])[None, :] >= nte[:, None]] = 123.0
    assert np.array_equal(clf.predict(pte, lengths=nte), labels)
    ptr, ntr = R.pad(tr)
    clf2 = SequenceClassifier(n_neighbors=3).fit(ptr, ytr, lengths=ntr)
    assert np.array_equal(clf2.predict(te), labels)
    res = clf.evaluate(te, y[45:])
    assert set(res) == {"accuracy", "predictions", "classification_report", "confusion_matrix"}
    assert res["accuracy"] == float(np.mean(labels == y[45:])) and np.array_equal(res["predictions"], labels)


def test_device_surface_takes_the_extraction_output_and_rejects_nan():
    """DtwIndex / dtw_pairwise on device tensors: the extraction's float32 seq converts exactly."""
    import torch
    from src.pipeline import DtwIndex, dtw_pairwise
    seqs, y = extracted()
    x32, n = R.pad([s.astype(np.float32) for s in seqs[:20]])
    x32 = x32.astype(np.float32)
    t32, tn = torch.as_tensor(x32).cuda(), torch.as_tensor(n).cuda()
    want = R.dtw_pairwise(x32[:6].astype(np.float64), n[:6], x32.astype(np.float64), n, 4)
    assert np.array_equal(bits(dtw_pairwise(t32[:6], tn[:6], t32, tn, window=4).cpu().numpy()), bits(want))
    assert np.array_equal(bits(dtw_pairwise(x32[:6], n[:6], x32, n, window=4).cpu().numpy()), bits(want))
    index = DtwIndex(t32, tn, y[:20], 3, window=4)
    got = index.query(t32[:6], tn[:6], self_offset=0)
    check_knn(tuple(t.cpu().numpy() for t in got), R.knn_from_dist(want, 3, y[:20], self_offset=0))
    bad = x32.copy()
    bad[3, 0, 1] = np.nan
    with pytest.raises(ValueError):
        dtw_pairwise(bad[:6], n[:6], x32, n)
    with pytest.raises(ValueError):
        index.query(torch.as_tensor(bad).cuda(), tn)


def test_knn_call_in_a_graph():
    """One dsp_dtw_knn call (two launches per chunk, no allocation, no sync) captured in a graph and
    replayed twice: the eager call's bits."""
    import torch
    from src import _hip
    lib = _hip.lib()
    ref, lr, labels, q, lq, d = knn_case()
    want = R.knn_from_dist(d, 3, labels)
    t = [torch.as_tensor(np.ascontiguousarray(x)).cuda() for x in (ref, lr.astype(np.int32), labels, q, lq.astype(np.int32))]
    (Nr, Tr, F), (Nq, Tq, _), k = ref.shape, q.shape, 3
    idx = torch.empty((Nq, k), dtype=torch.int32, device="cuda")
    dist = torch.empty((Nq, k), dtype=torch.float64, device="cuda")
    pred = torch.empty(Nq, dtype=torch.int32, device="cuda")
    nbytes = lib.dsp_dtw_workspace_bytes(Nr, Nq, Tr, Tq, F, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def call():
        rc = lib.dsp_dtw_knn(_hip.ptr(t[0]), _hip.ptr(t[1]), _hip.ptr(t[2]), Nr, Tr, _hip.ptr(t[3]), _hip.ptr(t[4]), Nq,
                             Tq, F, -1, k, -1, 4, _hip.ptr(idx), _hip.ptr(dist), _hip.ptr(pred), _hip.ptr(ws), nbytes,
                             _hip.stream_handle())
        assert rc == 0

    call()
    torch.cuda.synchronize()
    eager = (idx.cpu().numpy(), dist.cpu().numpy(), pred.cpu().numpy())
    check_knn(eager, want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        idx.fill_(-5)
        dist.fill_(-5.0)
        pred.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        check_knn((idx.cpu().numpy(), dist.cpu().numpy(), pred.cpu().numpy()), eager)


def _write_wav(path, data, width=2, channels=1, sr=44100):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(data).tobytes())


@pytest.fixture()
def dataset_dir(tmp_path):
    """The small synthetic WAV directory of tests/test_gpu_dataset.py (a copy of its helper)."""
    from src.synth import make_clip
    for c in range(3):
        d = tmp_path / ("w%d" % c)
        d.mkdir()
        for j in range(5):
            x = make_clip(2000 + 10 * c + j, n_samples=36000 + 1013 * j, label=c, n_classes=3)
            if c == 2 and j == 4:  # 8-bit file: same samples >> 8, offset 128
                _write_wav(d / ("s%d.wav" % j), ((x.astype(np.int32) >> 8) + 128).astype(np.uint8), width=1)
            else:
                _write_wav(d / ("s%d.wav" % j), x)
    with wave.open(str(tmp_path / "w0" / "zz_bad.wav"), "wb") as w:  # 24-bit: the reference raises
        w.setnchannels(1)
        w.setsampwidth(3)
        w.setframerate(44100)
        w.writeframes(b"\0" * 300)
    return str(tmp_path)


def test_compare_with_dtw(dataset_dir):
    """compare(dtw=True): the three reference rows unchanged, plus 'KNN-DTW' whose sequence accuracy
    is the reference restatement's on the unpadded (E, ZCR) sequences of the same split."""
    import compare_feature_methods as cfm
    from sklearn.model_selection import train_test_split
    base = cfm.compare(dataset_dir)
    res = cfm.compare(dataset_dir, dtw=True)
    assert list(base) == ["KNN", "SVM", "Decision Tree"] and list(res) == ["KNN", "SVM", "Decision Tree", "KNN-DTW"]
    assert {k: res[k] for k in base} == base
    row = res["KNN-DTW"]
    assert row["statistical"] == res["KNN"]["statistical"] and row["diff"] == row["sequence"] - row["statistical"]
    _, X_seq, y, lengths = cfm.load_both_methods(dataset_dir)
    tr, te = train_test_split(np.arange(len(y)), test_size=0.2, random_state=42, stratify=y)
    frames = np.concatenate([X_seq[i, :lengths[i]] for i in tr])
    mean, std = frames.mean(axis=0), frames.std(axis=0)
    std = np.where(std == 0, 1.0, std)
    a, la = R.pad([(X_seq[i, :lengths[i]] - mean) / std for i in te])
    b, lb = R.pad([(X_seq[i, :lengths[i]] - mean) / std for i in tr])
    classes, codes = np.unique(y[tr], return_inverse=True)
    _, _, pred = R.knn_from_dist(R.dtw_pairwise(a, la, b, lb, -1), 3, codes)
    assert row["sequence"] == float(np.mean(classes[pred] == y[te]))
