"""GPU tests of csrc/pitch.hip (dsp_pitch_track) through the bare C ABI, and of the Python surface on it.
Every integer is compared with the numpy restatement of tests/pitch_reference.py by assert_array_equal:
the track is defined exactly, so there is no tolerance and no frame is left out."""
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import crop_frame_cases as C
import pitch_reference as P
from crop_frame_cases import Guarded, _write_wav, pack

pytestmark = pytest.mark.gpu

FILL = (-9, -7, -7)  # lag, peak, r0 before the launch


def track_raw(pcm_t, off_t, B, max_len, L, S, lo, hi, se, nf, status, stride, ld):
    """dsp_pitch_track on device tensors -> (lag, peak, r0, frames on the plain path)."""
    import torch
    from src import _hip
    lib = _hip.lib()
    out = [Guarded((B, ld), dt, f) for dt, f in zip((torch.int32, torch.int64, torch.int64), FILL)]
    nbytes = lib.dsp_pitch_workspace_bytes(B, max_len, L, S, lo, hi)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0x55, dtype=torch.uint8, device="cuda")
    rc = lib.dsp_pitch_track(_hip.ptr(pcm_t), _hip.ptr(off_t), B, max_len, L, S, lo, hi, _hip.ptr(se), _hip.ptr(nf),
                             _hip.ptr(status), stride, *[_hip.ptr(o.view) for o in out], ld, _hip.ptr(ws), nbytes,
                             _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    return tuple(o.get() for o in out) + (int(ws[:4].view(torch.int32).item()),)


def track_given(clips, crops, L, S, lo, hi, **kw):
    """Hand-made clips with their crops given directly (crop_frame_cases.given, whose keywords these are)."""
    g = C.given(clips, crops, L, S, **kw)
    got = track_raw(g.pcm, g.off, g.B, g.max_len, L, S, lo, hi, *g.fields, g.stride, g.ld)
    want = P.track_batch(clips, g.se, g.nf, g.skip, L, S, lo, hi, g.ld, FILL)
    return got, want, (g.se, g.nf, g.status)


def wide_frames(clips, se, nf, status, L, S, ld):
    """Frames that the definition sends to the plain path: a centred sample outside [-32896, 32640)."""
    n = 0
    for b, x in enumerate(clips):
        if status[b] & 0xFF:
            continue
        y = np.asarray(x, np.int64) - P.centre(x)
        for t in range(min(int(nf[b]), ld)):
            f = P.frame(y, int(se[b][0]), int(se[b][1]), t, L, S)
            n += bool(((f >= 32640) | (f < -32896)).any())
    return n


def same(got, want):
    for g, w, name in zip(got, want, ("lag", "peak", "r0")):
        assert_array_equal(g, w, err_msg=name)


@functools.lru_cache(maxsize=None)
def synthetic(L, S):
    """64 synthetic clips of 0.25 s through a real dsp_extract_features call: the packed rows stay on
    the device, the crops come back for the reference."""
    import torch
    from src.pipeline import FeatureExtractor
    from src.synth import make_clip
    clips = [make_clip(500 + j, n_samples=11025) for j in range(64)]
    pcm, off = pack(clips)
    pcm_t, off_t = torch.as_tensor(pcm).to("cuda"), torch.as_tensor(off).to("cuda")
    fx = FeatureExtractor(L, S, "hamming", True)
    rows = fx(pcm_t, off_t, max_len=11025)["rows"].clone()
    torch.cuda.synchronize()
    return clips, pcm_t, off_t, rows, rows.cpu().numpy()


@pytest.mark.parametrize("L,S,lo,hi", ((1102, 441, 110, 735), (1024, 512, 1, 1023), (64, 16, 2, 63), (100, 37, 50, 50)))
def test_synthetic_clips(L, S, lo, hi):
    clips, pcm_t, off_t, rows, h = synthetic(L, S)
    se, nf, status = h[:, 15:17], h[:, 17], h[:, 18]
    assert ((status & 0xFF) == 0).all() and nf.min() >= 1 and (nf == [P.frame_count(e - s, L, S) for s, e in se]).all()
    ld = int(nf.max())
    want = P.track_batch(clips, se, nf, status, L, S, lo, hi, ld, FILL)
    assert (want[0][:, 0] >= lo).all() and (want[1] != FILL[1]).sum() == nf.sum()
    # the packed 76-byte rows straight in
    got = track_raw(pcm_t, off_t, 64, 11025, L, S, lo, hi, rows[:, 15:], rows[:, 17:], rows[:, 18:], 19, ld)
    same(got, want)
    assert got[3] == 0  # no full-scale sample: every frame on the matrix cores
    # the same as separate arrays
    sep = [rows[:, 15:17].contiguous(), rows[:, 17].contiguous(), rows[:, 18].contiguous()]
    same(track_raw(pcm_t, off_t, 64, 11025, L, S, lo, hi, *sep, 0, ld), want)


def edge_batch():
    """Hand-made clips and crops at L = 1102, S = 441 (docstring of test_edge_clips)."""
    rng = np.random.default_rng(11)
    clips, crops = [], []
    clips.append(P.tie_clip()), crops.append((0, 2204))  # 0
    clips.append(np.full(3000, 1234, np.int16)), crops.append((0, 3000))  # 1: constant
    x = np.zeros(3000, np.int16)
    x[[10, 310]] = [1000, -1000]
    clips.append(x), crops.append((0, 1102))  # 2: r(300) < 0, every other r = 0
    x = np.full(3000, 32767, np.int16)
    x[1500] = -32768
    clips.append(x), crops.append((0, 3000))  # 3
    x = (20000 + rng.integers(-300, 300, 4002)).astype(np.int16)
    x[[700, 1900, 3500]] = [-32768, 32767, -32768]
    x[[900, 2500]] = 32767
    clips.append(x), crops.append((0, 4002))  # 4: y leaves int16
    clips.append(rng.integers(-9000, 9000, 3333).astype(np.int16)), crops.append((301, 2906))  # 5: odd crop, odd clip start
    clips.append(rng.integers(-9000, 9000, 2001).astype(np.int16)), crops.append((100, 601))  # 6: one zero-padded frame
    for top, low in ((32511, -32767), (32512, -32768)):  # 7, 8: y = 32639 is the last int8 high digit, 32640 is not
        x = np.full(4000, -128, np.int16)
        x[100], x[2000] = top, low
        clips.append(x), crops.append((0, 4000))
    clips.append(rng.integers(-32000, 32001, 5000).astype(np.int16)), crops.append((0, 5000))  # 9: loud noise
    clips.append(np.where(np.arange(2500) % 2 == 0, 1000, -1000).astype(np.int16)), crops.append((0, 2500))  # 10
    return clips, crops


def test_edge_clips():
    """The tie clip (200 wins), a constant clip (lag_min, 0, 0 everywhere), a frame with no positive r,
    +32767 with one -32768, a DC offset of 20000 with full-scale excursions (y leaves int16), a crop
    from an odd sample of a clip at an odd offset, a crop shorter than L, the two sides of the high
    digit's int8 limit, full-scale noise and an alternating clip: one launch, both paths taken."""
    clips, crops = edge_batch()
    L, S, lo, hi = 1102, 441, 110, 735
    got, want, (se, nf, status) = track_given(clips, crops, L, S, lo, hi, lead=3)
    same(got, want)
    lag, peak, r0 = got[:3]
    assert (lag[0, 0], peak[0, 0], r0[0, 0]) == (200, 1000000, 3000000)
    assert (lag[1, :nf[1]] == lo).all() and not peak[1, :nf[1]].any() and not r0[1, :nf[1]].any()
    assert (lag[2, 0], peak[2, 0], r0[2, 0]) == (lo, 0, 2000000)
    assert P.centre(clips[4]) > 19000 and np.abs(clips[4].astype(np.int64) - P.centre(clips[4])).max() > 40000
    assert nf[6] == 1 and nf[5] > 1 and crops[5][0] % 2 == 1
    n_wide = wide_frames(clips, se, nf, status, L, S, lag.shape[1])
    assert got[3] == n_wide and 0 < n_wide < nf.sum() - 20
    assert wide_frames(clips[7:8], se[7:8], nf[7:8], status[7:8], L, S, 8) == 0
    assert wide_frames(clips[8:9], se[8:9], nf[8:9], status[8:9], L, S, 8) == 1
    assert wide_frames(clips[9:10], se[9:10], nf[9:10], status[9:10], L, S, 16) == 0
    assert P.voiced(peak[10, :nf[10]], r0[10, :nf[10]]).all() and (lag[10, :nf[10]] == lo).all()


def test_tie_rule_and_single_lags():
    """The tie clip with lag_min = 201 returns 300; the alternating clip at the single odd lag 51 has
    r < 0, and between 50 and 52 returns 50."""
    tie = [P.tie_clip()]
    got, want, _ = track_given(tie, [(0, 2204)], 1102, 441, 201, 735)
    same(got, want)
    assert (got[0][0, 0], got[1][0, 0]) == (300, 1000000)
    got, want, _ = track_given(tie, [(0, 2204)], 1102, 441, 301, 1101)
    same(got, want)
    assert (got[0][0, 0], got[1][0, 0]) == (500, 1000000)
    alt = [np.where(np.arange(400) % 2 == 0, 1000, -1000).astype(np.int16)]
    got, want, _ = track_given(alt, [(0, 400)], 100, 37, 51, 51)
    same(got, want)
    assert (got[0][0] == 51).all() and (got[1][0] < 0).all() and not P.voiced(got[1], got[2]).any()
    got, want, _ = track_given(alt, [(0, 400)], 100, 37, 50, 52)
    same(got, want)
    assert (got[0][0] == 50).all() and (got[1][0] > 0).all()


def test_short_ld_failed_clips_and_bad_crops():
    """ld smaller than nf; a failing status between two good ones (its rows keep the fill value) and a
    status with only flag bits set (processed); crops that do not lie inside their clip, a clip longer
    than max_len and n_frames below 1 write nothing; an empty crop with one frame is processed."""
    rng = np.random.default_rng(12)
    clips = [rng.integers(-5000, 5000, 3000 + 7 * j).astype(np.int16) for j in range(6)]
    crops = [(0, 3000), (5, 2900), (11, 3014), (0, 3021), (-1, 2000), (100, 3036)]
    status = [0, 3, 0x100, 0, 0, 0]
    got, want, (se, nf, st) = track_given(clips, crops, 1102, 441, 110, 735, status=status, ld=2,
                                          untouched=(4, 5))  # a negative start, an end behind the clip
    assert nf.min() > 2
    same(got, want)
    assert (got[0][4:] == FILL[0]).all()
    assert (got[0][1] == FILL[0]).all() and (got[1][1] == FILL[1]).all() and (got[0][[0, 2, 3]] != FILL[0]).all()
    # a clip longer than max_len is left alone like a failed one: n_frames of 0 writes nothing either
    got, want, _ = track_given(clips[:3], crops[:3], 1102, 441, 110, 735, n_frames=[3, 0, 6], status=[0, 0, 0], ld=6)
    same(got, want)
    assert (got[0][1] == FILL[0]).all() and (got[0][0, 3:] == FILL[0]).all()
    # every condition of the gate in one batch (crop_frame_cases.gate_batch), as separate arrays and as rows
    for stride in (0, 19):
        got, want, (se, nf, st) = track_given(lo=2, hi=63, stride=stride, **C.gate_batch())
        same(got, want)
        for g, fill in zip(got, FILL):
            assert (g[C.GATE_UNTOUCHED] == fill).all() and (g[8, 1:] == fill).all()
        assert (got[0][[0, 2]] >= 2).all() and (got[2][[0, 2]] > 0).all()
        assert (got[0][8, 0], got[1][8, 0], got[2][8, 0]) == (2, 0, 0)  # the empty crop's one all-zero frame


def test_longest_frames_full_scale():
    """L = 4096 with every lag 1 .. 4095 on full-scale noise below the int8 limit: sixteen lag tiles,
    the int32 accumulators at their largest."""
    rng = np.random.default_rng(13)
    clips = [rng.integers(-32000, 32001, 11025).astype(np.int16), rng.integers(29000, 31001, 9000).astype(np.int16) *
             rng.choice([-1, 1], 9000).astype(np.int16)]
    got, want, (se, nf, status) = track_given(clips, [(0, 11025), (3, 8999)], 4096, 1024, 1, 4095)
    same(got, want)
    assert got[3] == wide_frames(clips, se, nf, status, 4096, 1024, got[0].shape[1]) == 0
    assert got[2].max() > 4096 * 30000 ** 2 * 0.9


@functools.lru_cache(maxsize=None)
def tracker_case():
    import torch
    from src.pipeline import FeatureExtractor, PitchTracker
    clips, pcm_t, off_t, rows, h = synthetic(1102, 441)
    fx = FeatureExtractor(1102, 441, "hamming", True)
    out = fx(pcm_t, off_t, max_len=11025)
    tracker = PitchTracker(1102, 441, 44100)
    res = {k: v.cpu().numpy() for k, v in tracker(pcm_t, out, off_t, max_len=11025).items()}
    torch.cuda.synchronize()
    return clips, h, tracker, res


def test_pitch_tracker():
    clips, h, tracker, res = tracker_case()
    se, nf, status = h[:, 15:17], h[:, 17], h[:, 18]
    ld = tracker.frames(11025)
    assert res["lag"].shape == (64, ld) and ld >= nf.max() and tracker.plain_frames() == 0
    want = P.track_batch(clips, se, nf, status, 1102, 441, 110, 735, ld, (0, 0, 0))
    same((res["lag"], res["peak"], res["r0"]), want)
    voiced = P.voiced(want[1], want[2])
    assert_array_equal(res["voiced"], voiced)
    assert_array_equal(res["f0"].view(np.uint64), P.f0(want[0], voiced, 44100).view(np.uint64))
    inside = np.arange(ld)[None, :] < nf[:, None]
    assert voiced.sum() > 100 and (~voiced & inside).sum() > 0 and not voiced[~inside].any()
    with pytest.raises(ValueError):
        tracker(np.zeros((2, 4000), np.int32), {"rows": None})


def test_extract_both_with_pitch(tmp_path):
    """extract_both(pitch=True) on 3 x 4 WAV files: the 15 columns and the (E, ZCR) sequences are those
    of the default call, bit for bit, the default call is what the extractor's raw outputs give, and
    the five new columns and the f0 sequence column equal numpy's on the reference track."""
    import torch
    from src.audio_processing import load_wav_pcm
    from src.dataset import PCMDataset
    from src.pipeline import FeatureExtractor
    C.wav_tree(tmp_path, 4, 4000)
    ds = PCMDataset(str(tmp_path))
    X15, y, seq2, lengths = ds.extract_both(1102, 441)
    X20, y2, seq3, lengths2 = ds.extract_both(1102, 441, pitch=True)
    assert X15.shape == (12, 15) and X20.shape == (12, 20) and seq2.shape[2] == 2 and seq3.shape == seq2.shape[:2] + (3,)
    assert_array_equal(X20[:, :15].view(np.uint64), X15.view(np.uint64))
    assert_array_equal(seq3[:, :, :2].view(np.uint64), seq2.view(np.uint64))
    assert_array_equal(y, y2)
    assert_array_equal(lengths, lengths2)
    clips = [load_wav_pcm(f)[0] for f, _ in ds.files]
    pcm, off = pack(clips)
    fx = FeatureExtractor(1102, 441, "hamming", True, return_sequences=True)
    out = {k: v.cpu().numpy() for k, v in fx(torch.as_tensor(pcm).to("cuda"), off, max_len=int(np.diff(off).max())).items()}
    assert ((out["status"] & 0xFF) == 0).all()
    width = int(out["n_frames"].max())
    assert_array_equal(X15.view(np.uint64), out["feat"].astype(np.float64).view(np.uint64))
    assert_array_equal(seq2.view(np.uint64), out["seq"][:, :width][:, :, [0, 2]].astype(np.float64).view(np.uint64))
    assert_array_equal(lengths, out["n_frames"])
    lag, peak, r0 = P.track_batch(clips, out["start_end"], out["n_frames"], out["status"], 1102, 441, 110, 735, width, (0, 0, 0))
    voiced = P.voiced(peak, r0)
    f0 = P.f0(lag, voiced, 44100)
    assert_array_equal(seq3[:, :, 2].view(np.uint64), f0.view(np.uint64))
    stats = np.stack([P.f0_stats(a, b) for a, b in zip(f0, voiced)])
    assert_array_equal(X20[:, 15:].view(np.uint64), stats.view(np.uint64))
    assert voiced.any(axis=1).all() and (stats[:, 0] > 60).all()
    # 16-bit stereo whose channel sums need int32: the track takes int16 only
    _write_wav(tmp_path / "w0" / "stereo.wav", np.repeat(np.random.default_rng(5).integers(-30000, 30000, (30000, 1)), 2, axis=1).astype(np.int16), channels=2)
    wide = PCMDataset(str(tmp_path))
    assert len(wide.parts) == 2
    with pytest.raises(ValueError):
        wide.extract_both(1102, 441, pitch=True)
    assert wide.extract_both(1102, 441)[0].shape[1] == 15


def test_knn_on_f0_statistics_end_to_end():
    """300 labelled synthetic clips of 1 s: the five f0 statistics of the device track are the reference
    track's bit for bit, so the 3-NN on their z-scores (80/20 stratified split, random_state 42) predicts
    the same labels and reaches the reference's accuracy exactly."""
    import torch
    from sklearn.model_selection import train_test_split
    from src.feature_extraction import normalize_features
    from src.models import create_classifier
    from src.pipeline import FeatureExtractor, PitchTracker, f0_statistics
    from src.synth import make_batch
    pcm, y = make_batch(300, base_seed=7, with_labels=True)
    pcm_t = torch.as_tensor(pcm).to("cuda")
    out = FeatureExtractor(1102, 441, "hamming", True)(pcm_t)
    tracker = PitchTracker(1102, 441, 44100)
    res = {k: v.cpu().numpy() for k, v in tracker(pcm_t, out).items()}
    h = out["rows"].cpu().numpy()
    se, nf, status = h[:, 15:17], h[:, 17], h[:, 18]
    assert ((status & 0xFF) == 0).all()
    ld = res["lag"].shape[1]
    want = P.track_batch(list(pcm), se, nf, status, 1102, 441, 110, 735, ld, (0, 0, 0))
    same((res["lag"], res["peak"], res["r0"]), want)
    voiced = P.voiced(want[1], want[2])
    ref_stats = np.stack([P.f0_stats(a, b) for a, b in zip(P.f0(want[0], voiced, 44100), voiced)])
    dev_stats = f0_statistics(res["f0"], res["voiced"])
    assert_array_equal(dev_stats.view(np.uint64), ref_stats.view(np.uint64))

    def knn(X):
        tr, te, y_tr, y_te = train_test_split(X, y, test_size=0.2, random_state=42, stratify=y)
        tr, m, sd = normalize_features(tr)
        te, _, _ = normalize_features(te, m, sd)
        clf = create_classifier('knn', n_neighbors=3).fit(tr, y_tr)
        pred = np.asarray(clf.predict(te))
        return pred, float(np.mean(pred == y_te))

    (pred_d, acc_d), (pred_r, acc_r) = knn(dev_stats), knn(ref_stats)
    print("3-NN on the five f0 statistics: device %.4f, reference %.4f" % (acc_d, acc_r))
    assert_array_equal(pred_d, pred_r)
    assert acc_d == acc_r


def test_compare_with_pitch(tmp_path):
    """compare(pitch=True): every row on the 20-d matrix and the (E, ZCR, f0) sequences -- the KNN row
    is the 3-NN on extract_both(pitch=True)'s own matrices with the same split, and the DTW row gets
    F = 3; without the flag the rows are those of today's call."""
    import compare_feature_methods as cfm
    from sklearn.model_selection import train_test_split
    from src.feature_extraction import normalize_features
    from src.models import create_classifier
    C.wav_tree(tmp_path, 5, 5000, n_samples=30000)
    res = cfm.compare(str(tmp_path), dtw=True, pitch=True)
    assert list(res) == ["KNN", "SVM", "Decision Tree", "KNN-DTW"]
    X20, X_seq, y, lengths = cfm.load_both_methods(str(tmp_path), pitch=True)
    assert X20.shape == (15, 20) and X_seq.shape[2] == 3 and (X_seq[:, :, 2] >= 0).all() and X_seq[:, :, 2].max() > 60
    want = {}
    for name, X in (("statistical", X20), ("sequence", X_seq.reshape(15, -1))):
        tr, te, y_tr, y_te = train_test_split(X, y, test_size=0.2, random_state=42, stratify=y)
        tr, m, sd = normalize_features(tr)
        te, _, _ = normalize_features(te, m, sd)
        want[name] = float(create_classifier('knn', n_neighbors=3).fit(tr, y_tr).evaluate(te, y_te)['accuracy'])
    assert res["KNN"]["statistical"] == want["statistical"] and res["KNN"]["sequence"] == want["sequence"]
    assert res["KNN-DTW"]["statistical"] == want["statistical"] and 0.0 <= res["KNN-DTW"]["sequence"] <= 1.0
    X15, X_seq2, _, _ = cfm.load_both_methods(str(tmp_path))
    assert X15.shape == (15, 15) and X_seq2.shape[2] == 2
    assert_array_equal(X15.view(np.uint64), X20[:, :15].view(np.uint64))


def test_track_in_a_graph():
    """dsp_pitch_track (no allocation, no sync, its counter zeroed by a kernel) captured in a single-stream
    graph and replayed twice on the edge batch: the eager call's integers and plain-path count."""
    import torch
    from src import _hip
    lib = _hip.lib()
    clips, crops = edge_batch()
    L, S, lo, hi, B = 1102, 441, 110, 735, len(clips)
    pcm, off = pack(clips, lead=3)
    se = np.asarray(crops, np.int32)
    nf = np.array([P.frame_count(e - s, L, S) for s, e in se], np.int32)
    status = np.zeros(B, np.int32)
    ld, max_len = int(nf.max()), max(len(c) for c in clips)
    want = P.track_batch(clips, se, nf, status, L, S, lo, hi, ld, (-5, -5, -5))
    t = [torch.as_tensor(a).to("cuda") for a in (pcm, off, se, nf, status)]
    out = [torch.empty((B, ld), dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.int64)]
    nbytes = lib.dsp_pitch_workspace_bytes(B, max_len, L, S, lo, hi)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def call():
        rc = lib.dsp_pitch_track(_hip.ptr(t[0]), _hip.ptr(t[1]), B, max_len, L, S, lo, hi, _hip.ptr(t[2]), _hip.ptr(t[3]),
                                 _hip.ptr(t[4]), 0, *[_hip.ptr(o) for o in out], ld, _hip.ptr(ws), nbytes,
                                 _hip.stream_handle())
        assert rc == 0

    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        for o in out:
            o.fill_(-5)
        ws.fill_(0x55)
        g.replay()
        torch.cuda.synchronize()
        same([o.cpu().numpy() for o in out], want)
        assert int(ws[:4].view(torch.int32).item()) == wide_frames(clips, se, nf, status, L, S, ld)
