"""GPU tests of csrc/dtw_align.hip (dsp_dtw_align, dsp_dtw_dba_update) and the Python surface on it.
Everything is compared with the numpy restatements of tests/dtw_align_reference.py and
tests/dtw_reference.py on the raw bits and the raw integers: paths and templates are defined bit for
bit, so there is no tolerance and no pair is left out."""
import functools
import wave

import numpy as np
import pytest

import dtw_align_reference as A
import dtw_reference as R
from device_outputs import Guarded, _dev, bits, csr

pytestmark = pytest.mark.gpu


def align_raw(a, la, b, lb, start, members, window, with_dist=True, with_ranges=True):
    """dsp_dtw_align through the bare C ABI -> (dist, lo, hi), None where not asked for.  NaN follows
    both sequence buffers (a read past the last row would poison a result)."""
    import torch
    from src import _hip
    lib = _hip.lib()
    (Na, Ta, F), (Nb, Tb, _) = a.shape, b.shape
    P = len(members)
    ta = _dev(np.concatenate([a.reshape(-1), np.full(64, np.nan)]), torch.float64)
    tb = _dev(np.concatenate([b.reshape(-1), np.full(64, np.nan)]), torch.float64)
    tla, tlb = _dev(np.asarray(la, np.int32), torch.int32), _dev(np.asarray(lb, np.int32), torch.int32)
    ts, tm = _dev(np.asarray(start, np.int32), torch.int32), _dev(np.asarray(members, np.int32), torch.int32)
    gd, glo, ghi = Guarded((P,), torch.float64, -7.0), Guarded((P, Ta), torch.int32, -9), Guarded((P, Ta), torch.int32, -9)
    nbytes = lib.dsp_dtw_align_workspace_bytes(Na, P, Ta, Tb, F)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.dsp_dtw_align(_hip.ptr(ta), _hip.ptr(tla), Na, Ta, _hip.ptr(tb), _hip.ptr(tlb), Nb, Tb, F, window,
                           _hip.ptr(ts), _hip.ptr(tm), P, _hip.ptr(gd.view) if with_dist else None,
                           _hip.ptr(glo.view) if with_ranges else None, _hip.ptr(ghi.view) if with_ranges else None,
                           _hip.ptr(ws), nbytes, _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    dist, lo, hi = gd.get(), glo.get(), ghi.get()
    if not with_dist:
        assert (dist == -7.0).all()  # a NULL dist: nothing written
        dist = None
    if not with_ranges:
        assert (lo == -9).all() and (hi == -9).all()
        lo = hi = None
    return dist, lo, hi


def dba_raw(tmpl, lt, seqs, ls, start, members, window, with_inertia=True):
    """dsp_dtw_dba_update through the bare C ABI -> (tmpl_out, inertia or None)."""
    import torch
    from src import _hip
    lib = _hip.lib()
    (C, Tt, F), (N, Ts, _) = tmpl.shape, seqs.shape
    P = len(members)
    tt = _dev(np.concatenate([tmpl.reshape(-1), np.full(64, np.nan)]), torch.float64)
    tq = _dev(np.concatenate([seqs.reshape(-1), np.full(64, np.nan)]), torch.float64)
    tlt, tls = _dev(np.asarray(lt, np.int32), torch.int32), _dev(np.asarray(ls, np.int32), torch.int32)
    ts, tm = _dev(np.asarray(start, np.int32), torch.int32), _dev(np.asarray(members, np.int32).reshape(-1), torch.int32)
    go, gi = Guarded((C, Tt, F), torch.float64, -7.0), Guarded((C,), torch.float64, -7.0)
    nbytes = lib.dsp_dtw_align_workspace_bytes(C, P, Tt, Ts, F)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.dsp_dtw_dba_update(_hip.ptr(tt), _hip.ptr(tlt), C, Tt, _hip.ptr(tq), _hip.ptr(tls), N, Ts, F, window,
                                _hip.ptr(ts), _hip.ptr(tm) if P else None, P, _hip.ptr(go.view),
                                _hip.ptr(gi.view) if with_inertia else None, _hip.ptr(ws), nbytes, _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    out, inertia = go.get(), gi.get()
    if not with_inertia:
        assert (inertia == -7.0).all()
        inertia = None
    return out, inertia


def check_align(got, want):
    (gd, glo, ghi), (wd, wlo, whi) = got, want[:3]
    assert np.array_equal(bits(gd), bits(wd)), np.flatnonzero(bits(gd) != bits(wd))[:5]
    assert np.array_equal(glo, wlo), np.argwhere(glo != wlo)[:5]
    assert np.array_equal(ghi, whi), np.argwhere(ghi != whi)[:5]


def table_groups():
    """b[r] under a[(7 r) % 19]; then group 5 hands its members to group 6 (an empty group) and b[0]
    is also listed under a[3] (a b sequence under two a's)."""
    groups = [[r for r in range(37) if (7 * r) % 19 == c] for c in range(19)]
    groups[6] += groups[5]
    groups[5] = []
    groups[3].append(0)
    return groups


@functools.lru_cache(maxsize=None)
def table_reference(F, window):
    a, la, b, lb = R.table_case(F)
    start, members = csr(table_groups())
    return A.align(a, la, b, lb, start, members, window, "wavefront"), R.dtw_pairwise(a, la, b, lb, window)


@functools.lru_cache(maxsize=None)
def table_device(F, window):
    a, la, b, lb = R.table_case(F)
    start, members = csr(table_groups())
    return align_raw(a, la, b, lb, start, members, window)


@pytest.mark.parametrize("window", R.TABLE_WINDOWS)
@pytest.mark.parametrize("F", R.TABLE_F)
def test_align_table(F, window):
    """The pairwise case table (19 x 37 sequences, T = 70, lengths 1, 2, 31, 32, 33, 63, 64, 65, 70 on
    both sides): dist is dtw_reference.dtw_pairwise's entry, lo and hi are the restatement's."""
    want, full = table_reference(F, window)
    got = table_device(F, window)
    start, members = csr(table_groups())
    owner = np.repeat(np.arange(19), np.diff(start))
    assert np.array_equal(bits(got[0]), bits(full[owner, members]))
    assert start[5] == start[6] and (members == 0).sum() == 2
    check_align(got, want)


@pytest.mark.parametrize("window", R.TABLE_WINDOWS)
@pytest.mark.parametrize("F", R.TABLE_F)
def test_device_output_satisfies_the_path_invariants(F, window):
    """From the device's own output alone: the range invariants, the band, and the costs summed along
    the path reproduce D(end), so sqrt of the sum has dist's bits."""
    a, la, b, lb = R.table_case(F)
    dist, lo, hi = table_device(F, window)
    start, members = csr(table_groups())
    owner = np.repeat(np.arange(19), np.diff(start))
    for p, (c, r) in enumerate(zip(owner, members)):
        x, y = a[c, :la[c]], b[r, :lb[r]]
        path = A.path_of_ranges(lo[p], hi[p])
        t = x[path[:, 0]] - y[path[:, 1]]
        cost = (t * t)[:, 0]
        for f in range(1, F):
            cost = cost + (t * t)[:, f]
        d2 = np.cumsum(cost)[-1]
        assert bits(np.sqrt(d2)) == bits(dist[p])
        A.check_path(x, y, window, d2, lo[p], hi[p])


@pytest.mark.parametrize("window", (-1, 2))
@pytest.mark.parametrize("F", (1, 2))
def test_align_ties(F, window):
    """Values in {0, 1, 2}, every sequence against every sequence: many cells tie exactly, so this is
    the test of the diagonal / a-step / b-step order.  The pair (0,1,0) / (1,0,1) and its swap are among
    them and take different branches."""
    seqs = A.tie_case(F, 60 + F)
    x, n = R.pad(seqs)
    N = len(seqs)
    start, members = csr([list(range(N))] * N)
    want = A.align(x, n, x, n, start, members, window, "scalar")
    got = align_raw(x, n, x, n, start, members, window)
    check_align(got, want)
    p, q = (N - 2) * N + (N - 1), (N - 1) * N + (N - 2)
    assert bits(got[0][p]) == bits(got[0][q])
    fwd, back = A.path_of_ranges(got[1][p], got[2][p]), A.path_of_ranges(got[1][q], got[2][q])
    assert fwd.tolist() == [[0, 0], [0, 1], [1, 2], [2, 2]] and back.tolist() == fwd.tolist()
    assert back[:, ::-1].tolist() != fwd.tolist()


def test_align_wave_and_strip_edges():
    """Groups of 1, 63, 64, 65 and 130 members (a partial wave, a full one, a second tile, a third) under
    a sequences of 32, 33, 65, 1 and 64 frames (one strip, two with the first nearly empty, three): the
    path crosses strip boundaries and tiles of one group land on different waves."""
    rng = np.random.default_rng(71)
    F, la = 2, np.array([32, 33, 65, 1, 64], np.int32)
    a = rng.normal(0, 1, (5, 65, F))
    b, lb = R.case(9, 40, 70, F, seed=72)[2:]
    groups = [rng.integers(0, 40, g).tolist() for g in (1, 63, 64, 65, 130)]
    start, members = csr(groups)
    for window in (-1, 4):
        memo = {}
        dist, lo, hi = align_raw(a, la, b, lb, start, members, window)
        owner = np.repeat(np.arange(5), np.diff(start))
        for p, (c, r) in enumerate(zip(owner.tolist(), members.tolist())):
            if (c, r) not in memo:
                d2, path = A.align_pair(a[c, :la[c]], b[r, :lb[r]], window, "wavefront")
                memo[c, r] = (np.sqrt(d2),) + A.ranges(path, 65)
            wd, wlo, whi = memo[c, r]
            assert bits(dist[p]) == bits(wd) and np.array_equal(lo[p], wlo) and np.array_equal(hi[p], whi), (p, c, r)


def test_align_longest_sequences():
    """T = 1024: a of 1024 and 993 frames (32 strips; 32 with the first holding one frame), b of 1024,
    1000 and 1 frames, unconstrained and window = 40, against the wavefront form."""
    rng = np.random.default_rng(81)
    a, b = rng.normal(0, 1, (2, 1024, 2)), rng.normal(0, 1, (3, 1024, 2))
    la, lb = np.array([1024, 993], np.int32), np.array([1024, 1000, 1], np.int32)
    start, members = csr([[0, 1, 2], [2, 1, 0]])
    for window in (-1, 40):
        want = A.align(a, la, b, lb, start, members, window, "wavefront")
        assert np.isfinite(want[0]).all()
        check_align(align_raw(a, la, b, lb, start, members, window), want)


def test_invalid_input_gives_inf_and_minus_one():
    """A length of 0, a length above T (either side) and members entries out of range: +inf / -1, every
    other pair the restatement's; the padding is NaN (nothing outside a sequence's frames reaches a
    result), the guard rows stay (Guarded), a NULL dist or NULL ranges is honoured."""
    a, la, b, lb = (x.copy() for x in R.table_case(2))
    la[[2, 7]] = [0, 71]
    lb[[0, 20, 36]] = [71, 0, -1]
    for x, n in ((a, la), (b, lb)):
        for i in range(len(x)):
            if 1 <= n[i] <= 70:
                x[i, n[i]:] = np.nan
    groups = table_groups()
    groups[1] += [-1, 37, 1 << 30, -(1 << 31)]
    start, members = csr(groups)
    for window in (-1, 3):
        want = A.align(np.nan_to_num(a), la, np.nan_to_num(b), lb, start, members, window, "wavefront")
        bad = np.isinf(want[0])
        assert bad.sum() >= 4 + len(groups[2]) + len(groups[7]) and (~bad).sum() > 20
        assert (want[1][bad] == -1).all() and (want[2][bad] == -1).all()
        got = align_raw(a, la, b, lb, start, members, window)
        check_align(got, want)
        only_d = align_raw(a, la, b, lb, start, members, window, with_ranges=False)
        assert np.array_equal(bits(only_d[0]), bits(want[0])) and only_d[1] is None
        only_r = align_raw(a, la, b, lb, start, members, window, with_dist=False)
        assert only_r[0] is None and np.array_equal(only_r[1], want[1]) and np.array_equal(only_r[2], want[2])


def test_position_independence():
    """One pair in different lanes, tiles, groups and group chunks (1030 groups: two launches), and
    alone: the same bits and the same ranges."""
    rng = np.random.default_rng(91)
    x, y = rng.normal(0, 1, (45, 3)), rng.normal(0, 1, (70, 3))
    Na, Nb = 1030, 80
    for window in (-1, 5):
        d2, path = A.align_pair(x, y, window, "wavefront")
        wd, (wlo, whi) = np.sqrt(d2), A.ranges(path, 45)
        alone = align_raw(x[None], [45], y[None], [70], [0, 1], [0], window)
        assert bits(alone[0][0]) == bits(wd) and np.array_equal(alone[1][0], wlo) and np.array_equal(alone[2][0], whi)
        a, b = rng.normal(0, 1, (Na, 45, 3)), rng.normal(0, 1, (Nb, 70, 3))
        la, lb = rng.integers(1, 46, Na).astype(np.int32), rng.integers(1, 71, Nb).astype(np.int32)
        for c in (0, 5, 1025, 1029):
            a[c], la[c] = x, 45
        for r in (0, 41, 79):
            b[r], lb[r] = y, 70
        groups = [[] for _ in range(Na)]
        groups[0] = [0, 7, 79]
        groups[5] = [0] + rng.integers(1, 40, 62).tolist() + [41, 79] + rng.integers(1, 40, 5).tolist()  # lanes 0, 63; tile 2
        groups[700] = rng.integers(0, Nb, 3).tolist()
        groups[1025] = [41]
        groups[1029] = [3, 79]
        start, members = csr(groups)
        dist, lo, hi = align_raw(a, la, b, lb, start, members, window)
        hits = [start[0], start[0] + 2, start[5], start[5] + 63, start[5] + 64, start[1025], start[1029] + 1]
        for p in hits:
            assert bits(dist[p]) == bits(wd) and np.array_equal(lo[p], wlo) and np.array_equal(hi[p], whi), p


def dba_case(seed=101):
    """Three templates of lengths 1, 33 and 64 (Tt = 64) with 1, 65 and 0 members out of 66 sequences
    of 1 .. 70 frames, F = 2; one member has an invalid length."""
    rng = np.random.default_rng(seed)
    tmpl, lt = rng.normal(0, 1, (3, 64, 2)), np.array([1, 33, 64], np.int32)
    seqs, ls = R.case(9, 66, 70, 2, seed=seed + 1)[2:]
    ls[17] = 0
    start, members = csr([[65], list(range(65)), []])
    return tmpl, lt, seqs, ls, start, members


@pytest.mark.parametrize("window", (-1, 3))
def test_dba_update(window):
    tmpl, lt, seqs, ls, start, members = dba_case()
    want = A.dba_update(tmpl, lt, seqs, ls, start, members, window, "wavefront")
    out, inertia = dba_raw(tmpl, lt, seqs, ls, start, members, window)
    assert np.array_equal(bits(out), bits(want[0])), np.argwhere(bits(out) != bits(want[0]))[:5]
    assert np.array_equal(bits(inertia), bits(want[1]))
    assert np.array_equal(bits(out[2]), bits(tmpl[2])) and inertia[2] == 0.0  # no member: copied
    assert not out[0, 1:].any() and not out[1, 33:].any() and (inertia[:2] > 0).all()
    out2, none = dba_raw(tmpl, lt, seqs, ls, start, members, window, with_inertia=False)
    assert none is None and np.array_equal(bits(out2), bits(out))
    # a template with an invalid length, and one whose only member is invalid: copied, inertia 0.0
    lt2 = np.array([65, 33, 64], np.int32)
    start2, members2 = csr([[65], list(range(65)), [17]])
    want = A.dba_update(tmpl, lt2, seqs, ls, start2, members2, window, "wavefront")
    out, inertia = dba_raw(tmpl, lt2, seqs, ls, start2, members2, window)
    assert np.array_equal(bits(out), bits(want[0])) and np.array_equal(bits(inertia), bits(want[1]))
    assert np.array_equal(bits(out[[0, 2]]), bits(tmpl[[0, 2]])) and inertia[0] == 0.0 and inertia[2] == 0.0


def test_dba_fixed_point():
    """A class of identical sequences returns that sequence with inertia 0.0.  The values are float32
    ones, as the extraction's sequences are: nine of them sum exactly in fp64, so the division returns
    them (with full fp64 mantissas s + s + s already rounds)."""
    rng = np.random.default_rng(111)
    s = np.zeros((1, 40, 3))
    s[0, :37] = rng.normal(0, 1, (37, 3)).astype(np.float32)
    seqs = np.repeat(s, 9, axis=0)
    out, inertia = dba_raw(s, [37], seqs, [37] * 9, [0, 9], np.arange(9), -1)
    assert np.array_equal(bits(out), bits(s)) and inertia.tolist() == [0.0]


def test_dba_pair_chunks():
    """The pairs of one update run in chunks whose ranges and sums fit 128 MiB (5461 pairs at Tt = 1024,
    F = 2); the sums carry from chunk to chunk in list order.  8262 one-frame members under one template of 1000
    frames: every template frame is matched to the member's only frame, so acc is the sequential sum of
    the members, cnt their number, and D(end) the sequential sum of the costs along the template."""
    rng = np.random.default_rng(121)
    P, L, F = 8262, 1000, 2
    tmpl = np.zeros((1, 1024, F))
    tmpl[0, :L] = rng.normal(0, 1, (L, F))
    seqs = rng.normal(0, 1, (P, 1, F))
    acc = np.cumsum(seqs[:, 0, :], axis=0)[-1]
    want = np.zeros_like(tmpl)
    want[0, :L] = acc / np.float64(P)
    t = tmpl[0, None, :L, 0] - seqs[:, :, 0]
    c = t * t
    t = tmpl[0, None, :L, 1] - seqs[:, :, 1]
    c = c + t * t
    inert = np.cumsum(np.cumsum(c, axis=1)[:, -1])[-1]
    out, inertia = dba_raw(tmpl, [L], seqs, np.ones(P, np.int32), [0, P], np.arange(P), -1)
    assert np.array_equal(bits(out), bits(want)) and bits(inertia[0]) == bits(inert)


def test_dba_group_chunks():
    """1030 templates run as two launches of at most 1024 groups, each over its own run of the pair
    list: tiny sequences, groups of 0 to 2 members."""
    rng = np.random.default_rng(141)
    C, N = 1030, 50
    tmpl, lt = rng.normal(0, 1, (C, 5, 1)), rng.integers(1, 6, C).astype(np.int32)
    seqs, ls = rng.normal(0, 1, (N, 6, 1)), rng.integers(1, 7, N).astype(np.int32)
    start, members = csr([rng.integers(0, N, int(g)).tolist() for g in rng.integers(0, 3, C)])
    assert start[1024] < start[1030] and (np.diff(start) == 0).sum() > 100
    want = A.dba_update(tmpl, lt, seqs, ls, start, members, -1, "scalar")
    out, inertia = dba_raw(tmpl, lt, seqs, ls, start, members, -1)
    assert np.array_equal(bits(out), bits(want[0])) and np.array_equal(bits(inertia), bits(want[1]))


def test_dba_update_in_a_graph():
    """One dsp_dtw_dba_update call (no allocation, no sync) captured in a single-stream graph and
    replayed twice: the eager call's bits."""
    import torch
    from src import _hip
    lib = _hip.lib()
    tmpl, lt, seqs, ls, start, members = dba_case()
    want = A.dba_update(tmpl, lt, seqs, ls, start, members, 3, "wavefront")
    t = [_dev(tmpl, torch.float64), _dev(lt, torch.int32), _dev(seqs, torch.float64), _dev(ls, torch.int32),
         _dev(start, torch.int32), _dev(members, torch.int32)]
    (C, Tt, F), (N, Ts, _), P = tmpl.shape, seqs.shape, len(members)
    out = torch.empty((C, Tt, F), dtype=torch.float64, device="cuda")
    inertia = torch.empty(C, dtype=torch.float64, device="cuda")
    nbytes = lib.dsp_dtw_align_workspace_bytes(C, P, Tt, Ts, F)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def call():
        rc = lib.dsp_dtw_dba_update(_hip.ptr(t[0]), _hip.ptr(t[1]), C, Tt, _hip.ptr(t[2]), _hip.ptr(t[3]), N, Ts, F, 3,
                                    _hip.ptr(t[4]), _hip.ptr(t[5]), P, _hip.ptr(out), _hip.ptr(inertia), _hip.ptr(ws),
                                    nbytes, _hip.stream_handle())
        assert rc == 0

    call()
    torch.cuda.synchronize()
    eager = (out.cpu().numpy(), inertia.cpu().numpy())
    assert np.array_equal(bits(eager[0]), bits(want[0])) and np.array_equal(bits(eager[1]), bits(want[1]))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        out.fill_(-5.0)
        inertia.fill_(-5.0)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(eager[0]))
        assert np.array_equal(bits(inertia.cpu().numpy()), bits(eager[1]))


def class_sequences(seed=131):
    """3 classes x 7 sequences of 3 .. 40 frames, F = 2, the classes interleaved; labels 2, 7, 12."""
    rng = np.random.default_rng(seed)
    seqs, y = [], []
    for i in range(21):
        c, n = i % 3, int(rng.integers(3, 41))
        t = np.linspace(0, 1, n)[:, None]
        seqs.append(np.hstack([np.sin((c + 1) * 3 * t), 50.0 * t ** (c + 1)]) + rng.normal(0, 0.1, (n, 2)) * [1, 20.0])
        y.append(c * 5 + 2)
    lens = [len(s) for s in seqs]
    assert min(lens) >= 3 and max(lens) <= 40
    return seqs, np.array(y)


def test_template_classifier():
    from src.models import TemplateClassifier
    from src.pipeline import dtw_align, dtw_barycenter
    seqs, y = class_sequences()
    clf = TemplateClassifier(n_iter=3).fit(seqs, y)
    frames = np.concatenate(seqs)
    mean, std = frames.mean(axis=0), frames.std(axis=0)
    X, n = R.pad([(s - mean) / std for s in seqs])
    classes, codes = np.unique(y, return_inverse=True)
    tmpl, lt, inertia = A.template_fit(X, n, codes, 3)
    assert clf.templates_.shape == (3, X.shape[1], 2) and clf.inertia_.shape == (3, 3)
    assert np.array_equal(bits(clf.templates_), bits(tmpl)) and np.array_equal(clf.template_lengths_, lt)
    assert clf.template_lengths_.dtype == np.int32 and np.array_equal(bits(clf.inertia_), bits(inertia))
    queries = class_sequences(seed=132)[0]
    q, nq = R.pad([(s - mean) / std for s in queries])
    d = R.dtw_pairwise(q, nq, tmpl, lt, -1)
    idx, dist, pred = R.knn_from_dist(d, 1, np.arange(3))
    assert np.array_equal(clf.predict(queries), classes[pred])
    gd, gi = clf.kneighbors(queries)
    assert np.array_equal(gi, idx.astype(np.int64)) and np.array_equal(bits(gd), bits(dist))
    res = clf.evaluate(queries, class_sequences(seed=132)[1])
    assert res["accuracy"] == float(np.mean(classes[pred] == class_sequences(seed=132)[1]))
    # a band, and fewer candidates than members, follow the same rules
    clf2 = TemplateClassifier(n_iter=2, window=3, medoid_candidates=2, normalize=False).fit(X, y, lengths=n)
    t2, l2, i2 = A.template_fit(X, n, codes, 2, window=3, candidates=2)
    assert np.array_equal(bits(clf2.templates_), bits(t2)) and np.array_equal(clf2.template_lengths_, l2)
    assert np.array_equal(bits(clf2.inertia_), bits(i2))
    # the device surface under it: dtw_align with assign, dtw_barycenter's early stop
    assign = np.where(np.arange(21) % 3 == 1, -1, codes)
    dist, lo, hi, start, members = dtw_align(tmpl, lt, X, n, assign=assign)
    start, members = start.cpu().numpy(), members.cpu().numpy()
    assert start.tolist() == [0, 7, 7, 14] and members.tolist() == [i for c in (0, 2) for i in range(21) if i % 3 == c]
    check_align((dist.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()), A.align(tmpl, lt, X, n, start, members, -1))
    only = dtw_align(tmpl, lt, X, n, groups=(start, members), window=2, with_ranges=False)
    assert only[1] is None and np.array_equal(bits(only[0].cpu().numpy()), bits(A.align(tmpl, lt, X, n, start, members, 2)[0]))
    mem = np.flatnonzero(codes == 0)
    init = X[mem[0], :n[mem[0]]]
    bary, inert = dtw_barycenter(X[mem], n[mem], init, n_iter=30)
    want, winert = init[None], []
    for _ in range(30):
        new, i1 = A.dba_update(want, [len(init)], X[mem], n[mem], [0, len(mem)], np.arange(len(mem)))
        winert.append(i1[0])
        same = np.array_equal(bits(new), bits(want))
        want = new
        if same:
            break
    full = want
    for _ in range(30 - len(winert)):
        full = A.dba_update(full, [len(init)], X[mem], n[mem], [0, len(mem)], np.arange(len(mem)))[0]
    assert np.array_equal(bits(bary), bits(want[0])) and np.array_equal(bits(inert), bits(np.array(winert)))
    assert np.array_equal(bits(full), bits(want))  # stopping early changes nothing


def test_dtw_path_of_extracted_sequences():
    """dtw_path on two sequences from the extraction (float32 seq converts exactly)."""
    import torch
    from src.pipeline import FeatureExtractor, dtw_path
    from src.synth import make_batch
    out = FeatureExtractor(1102, 441, "hamming", True, return_sequences=True)(torch.as_tensor(make_batch(4), device="cuda"))
    seq, n = out["seq"].cpu().numpy(), out["n_frames"].cpu().numpy()
    assert ((out["status"].cpu().numpy() & 0xFF) == 0).all() and n.min() >= 1
    x, y = seq[0, :n[0]][:, [0, 2]].astype(np.float64), seq[3, :n[3]][:, [0, 2]].astype(np.float64)
    for window in (None, 3):
        d2, path = A.align_pair(x, y, -1 if window is None else window, "wavefront")
        gd, gp = dtw_path(seq[0, :n[0]][:, [0, 2]], torch.as_tensor(y), window=window)
        assert bits(gd) == bits(np.sqrt(d2)) and gp.dtype == np.int64 and np.array_equal(gp, path)
    assert gp[0].tolist() == [0, 0] and gp[-1].tolist() == [len(x) - 1, len(y) - 1]


def _write_wav(path, data, width=2, channels=1, sr=44100):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(data).tobytes())


@pytest.fixture()
def dataset_dir(tmp_path):
    """The small synthetic WAV directory that tests/test_gpu_dtw.py::test_compare_with_dtw builds (a
    copy of its helper)."""
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


def test_compare_with_dtw_template(dataset_dir):
    """compare(dtw=True, dtw_template=True): the rows of compare(dtw=True) unchanged, plus
    'DTW-template' whose sequence accuracy is the restatement's on the same split."""
    import compare_feature_methods as cfm
    from sklearn.model_selection import train_test_split
    base = cfm.compare(dataset_dir, dtw=True)
    res = cfm.compare(dataset_dir, dtw=True, dtw_template=True)
    assert list(base) == ["KNN", "SVM", "Decision Tree", "KNN-DTW"] and list(res) == list(base) + ["DTW-template"]
    assert {k: res[k] for k in base} == base
    row = res["DTW-template"]
    assert row["statistical"] == res["KNN"]["statistical"] and row["diff"] == row["sequence"] - row["statistical"]
    _, X_seq, y, lengths = cfm.load_both_methods(dataset_dir)
    lengths = np.asarray(lengths)
    tr, te = train_test_split(np.arange(len(y)), test_size=0.2, random_state=42, stratify=y)
    frames = np.concatenate([X_seq[i, :lengths[i]] for i in tr])
    mean, std = frames.mean(axis=0), frames.std(axis=0)
    std = np.where(std == 0, 1.0, std)
    a, la = R.pad([(X_seq[i, :lengths[i]] - mean) / std for i in te])
    b, lb = R.pad([(X_seq[i, :lengths[i]] - mean) / std for i in tr], T=X_seq.shape[1])
    classes, codes = np.unique(y[tr], return_inverse=True)
    tmpl, lt, _ = A.template_fit(b, lb, codes, 10)
    _, _, pred = R.knn_from_dist(R.dtw_pairwise(a, la, tmpl, lt, -1), 1, np.arange(len(classes)))
    assert row["sequence"] == float(np.mean(classes[pred] == y[te]))
