"""GPU tests of csrc/lpc.hip (dsp_lpc_autocorr, dsp_lpc_solve) through the bare C ABI, and of the Python
surface on it.  Every integer and every double is compared with the restatement of tests/lpc_reference.py
by assert_array_equal (doubles as their bit patterns): both halves are defined exactly, so there is no
tolerance and no frame is left out."""
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import crop_frame_cases as C
import lpc_reference as R
import pitch_reference as P
from crop_frame_cases import Guarded, _write_wav, pack

pytestmark = pytest.mark.gpu

FILL = -7  # r before the launch


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def autocorr_raw(pcm_t, off_t, B, max_len, L, S, p, table_t, se, nf, status, stride, ld):
    """dsp_lpc_autocorr on device tensors -> (r [B, ld, p + 1], the workspace's counter)."""
    import torch
    from src import _hip
    lib = _hip.lib()
    out = Guarded((B, ld, p + 1), torch.int64, FILL)
    nbytes = lib.dsp_lpc_workspace_bytes(B, max_len, L, S, p)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0x55, dtype=torch.uint8, device="cuda")
    rc = lib.dsp_lpc_autocorr(_hip.ptr(pcm_t), _hip.ptr(off_t), B, max_len, L, S, p, _hip.ptr(table_t), _hip.ptr(se),
                              _hip.ptr(nf), _hip.ptr(status), stride, _hip.ptr(out.view), ld, _hip.ptr(ws), nbytes,
                              _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    return out.get(), int(ws[:4].view(torch.int32).item())


def autocorr_given(clips, crops, L, S, p, table=None, want=None, **kw):
    """Hand-made clips with their crops given directly (crop_frame_cases.given, whose keywords these are);
    ``want``: a reference from an earlier call with the same clips, crops and table.
    -> (r, counter, reference, (se, nf, status))"""
    import torch
    g = C.given(clips, crops, L, S, **kw)
    table_t = None if table is None else torch.as_tensor(np.asarray(table)).to("cuda")
    got, count = autocorr_raw(g.pcm, g.off, g.B, g.max_len, L, S, p, table_t, *g.fields, g.stride, g.ld)
    if want is None:
        want = R.autocorr_batch(clips, g.se, g.nf, g.skip, L, S, p, table, g.ld, FILL)
    return got, count, want, (g.se, g.nf, g.status)


def solve_raw(r, p, Q):
    """dsp_lpc_solve on host rows r [n, p + 1] -> (a, k, err, reached, cep) with guards around each."""
    import torch
    from src import _hip
    r = np.ascontiguousarray(r, np.int64).reshape(-1, p + 1)
    n = len(r)
    r_t = torch.as_tensor(r).to("cuda")
    a, k = Guarded((n, p), torch.float64, -7.5), Guarded((n, p), torch.float64, -7.5)
    err, reached = Guarded((n,), torch.float64, -7.5), Guarded((n,), torch.int32, -9)
    cep = Guarded((n, Q), torch.float64, -7.5)
    rc = _hip.lib().dsp_lpc_solve(_hip.ptr(r_t), n, p, Q, _hip.ptr(a.view), _hip.ptr(k.view), _hip.ptr(err.view),
                                  _hip.ptr(reached.view), _hip.ptr(cep.view) if Q else None, _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    assert_array_equal(r_t.cpu().numpy(), r)
    return a.get(), k.get(), err.get(), reached.get(), cep.get()


def same_solution(got, want):
    for g, w, name in zip(got, want, ("a", "k", "err", "reached", "cep")):
        assert not np.isnan(np.asarray(g, np.float64)).any(), name
        assert_array_equal(g if name == "reached" else bits(g), w if name == "reached" else bits(w), err_msg=name)


def table_of(name, L):
    from src.pipeline import lpc_window
    return lpc_window({"none": "rectangular"}.get(name, name), L)


SHAPES = ((1102, 441, 12), (64, 16, 8), (33, 7, 32), (2, 1, 1), (4096, 2048, 32))


@functools.lru_cache(maxsize=None)
def shape_clips(L):
    """The clips and crops of one shape: six synthetic clips of 1 s at L = 1102 (crops from odd and even
    samples, one ending inside its last frame), the first samples of them at the small shapes, one clip of
    12 288 samples at L = 4096."""
    from src.synth import make_clip
    if L == 4096:
        return [make_clip(31, label=3)[:12288]], [(1, 12288)]
    if L == 1102:
        clips = [make_clip(7 + i, label=i % 10) for i in range(6)]
        return clips, [(137 + b, 44100 - 301 * b) for b in range(6)]
    n = {64: 2400, 33: 700, 2: 40}[L]
    clips = [make_clip(7 + i, label=i % 10)[9000:9000 + n + 11 * i] for i in range(6)]
    return clips, [(b, n + 11 * b - (b & 1)) for b in range(6)]


@functools.lru_cache(maxsize=None)
def shape_reference(L, S, p, window):
    clips, crops = shape_clips(L)
    se = np.asarray(crops, np.int32)
    nf = np.array([P.frame_count(e - s, L, S) for s, e in se], np.int32)
    return R.autocorr_batch(clips, se, nf, np.zeros(len(clips), np.int32), L, S, p, table_of(window, L), int(nf.max()), FILL)


@pytest.mark.parametrize("window", ("none", "hamming", "hanning"))
@pytest.mark.parametrize("L,S,p", SHAPES)
def test_r_against_the_restatement(L, S, p, window):
    """Every shape with every table; the clips behind 0 .. 7 samples of another owner, so that frames
    start on odd samples and off 16-byte boundaries (all eight leads at the two smallest shapes and
    with the Hamming table at 1102, three elsewhere)."""
    clips, crops = shape_clips(L)
    want = shape_reference(L, S, p, window)
    assert (want[:, 0, 0] > 0).all() or not np.any(table_of(window, L))  # (hanning(2) is all zero)
    leads = range(8) if L <= 33 or (L == 1102 and window == "hamming") else (0, 3, 6)
    for lead in leads:
        got, count, _, _ = autocorr_given(clips, crops, L, S, p, table_of(window, L), lead=lead, want=want)
        assert_array_equal(got, want, err_msg="lead %d" % lead)
        assert count == 0


def test_lower_orders_are_prefixes():
    """Orders inside one order class and across classes (1, 5, 12, 13, 17, 25) equal the first lags of the
    order-32 reference."""
    clips, crops = shape_clips(64)
    want = shape_reference(64, 16, 32, "hamming")
    for p in (1, 5, 12, 13, 17, 25, 32):
        got, _, _, _ = autocorr_given(clips, crops, 64, 16, p, table_of("hamming", 64), lead=1, want=want[:, :, :p + 1])
        assert_array_equal(got, want[:, :, :p + 1], err_msg="order %d" % p)


def test_short_tails():
    """Crops that end inside the last frames, with fewer valid samples than the order, and frames wholly
    behind the crop (n_frames given by hand): zeros behind the last valid sample, an all-zero r for an
    empty frame; a crop of four samples in a frame of 64."""
    clips, _ = shape_clips(64)
    crops = [(0, 100), (3, 101), (5, 9), (0, 64), (1, 66), (7, 2000)]
    nfs = [8, 7, 1, 1, 2, 3]
    for window in ("none", "hamming"):
        got, count, want, _ = autocorr_given(clips, crops, 64, 16, 8, table_of(window, 64), n_frames=nfs, lead=5)
        assert_array_equal(got, want)
        assert not got[0, 7].any() and not got[0, 6, 4:].any() and got[0, 6, 0] > 0  # four valid samples in frame 6
        assert (got[2, 1:] == FILL).all() and (got[5, 3:] == FILL).all() and count == 0


def test_edge_tables():
    """An all-zero table gives r = 0 everywhere; entries below 0 and above 32768 are clamped (the result
    is that of the clamped table, and a table of 40 000 everywhere that of no table)."""
    clips, crops = shape_clips(64)
    L, S, p = 64, 16, 8
    got, _, want, (se, nf, _) = autocorr_given(clips, crops, L, S, p, np.zeros(L, np.int32))
    assert_array_equal(got, want)
    inside = np.arange(got.shape[1])[None, :] < nf[:, None]
    assert not got[inside].any() and (got[~inside] == FILL).all()
    wild = table_of("hamming", L).copy()
    wild[::3] = np.resize(np.array([-5, 40000, -(2 ** 31), 2 ** 31 - 1, 32769, -1, 65536, -32768], np.int32), len(wild[::3]))
    got, _, want, _ = autocorr_given(clips, crops, L, S, p, wild)
    assert_array_equal(got, want)
    clamped, _, _, _ = autocorr_given(clips, crops, L, S, p, np.clip(wild, 0, 32768), want=want)
    assert_array_equal(clamped, want)
    big, _, _, _ = autocorr_given(clips, crops, L, S, p, np.full(L, 40000, np.int32), want=shape_reference(L, S, p, "none"))
    assert_array_equal(big, shape_reference(L, S, p, "none"))


def test_full_scale_and_constant_clips():
    """A +32767 / -32768 square wave, a clip with a DC offset of 20 000 and full-scale excursions (y leaves
    int16: |z| up to 52 768), full-scale noise and a constant clip (all r = 0), windowed and not: the same
    r as the restatement, the largest products and sums of the plan, and no frame on a fallback path."""
    rng = np.random.default_rng(11)
    sq = np.where((np.arange(5000) // 7) % 2 == 0, 32767, -32768).astype(np.int16)
    dc = (20000 + rng.integers(-300, 300, 4002)).astype(np.int16)
    dc[[700, 1900, 3500]] = [-32768, 32767, -32768]
    dc[[900, 2500]] = 32767
    clips = [sq, dc, rng.integers(-32768, 32768, 5000).astype(np.int16), np.full(3000, 1234, np.int16),
             np.full(2500, -32768, np.int16)]
    crops = [(0, 5000), (1, 4002), (3, 4999), (0, 3000), (0, 2500)]
    assert P.centre(dc) > 19000 and np.abs(dc.astype(np.int64) - P.centre(dc)).max() > 40000
    for L, S, p, window in ((1102, 441, 12, "none"), (1102, 441, 12, "hamming"), (4096, 1024, 32, "none")):
        got, count, want, (se, nf, _) = autocorr_given(clips, crops, L, S, p, table_of(window, L), lead=3)
        assert_array_equal(got, want)
        assert count == R.wide_frames() == 0
        assert not got[3, :nf[3]].any() and not got[4, :nf[4]].any()
        if window == "none":
            assert got[0, 0, 0] > L * 32767 ** 2 * 0.99


def test_untouched_rows():
    """ld smaller than nf; a failing status between two good ones (its rows keep the fill value) and a
    status with only flag bits set (processed); crops that do not lie inside their clip, a clip longer
    than max_len and n_frames below 1 write nothing; an empty crop with one frame is processed."""
    import torch
    rng = np.random.default_rng(12)
    clips = [rng.integers(-5000, 5000, 3000 + 7 * j).astype(np.int16) for j in range(6)]
    crops = [(0, 3000), (5, 2900), (11, 3014), (0, 3021), (-1, 2000), (100, 3036)]
    ham = table_of("hamming", 1102)
    got, count, want, (se, nf, st) = autocorr_given(clips, crops, 1102, 441, 12, ham, status=[0, 3, 0x100, 0, 0, 0], ld=2,
                                                    untouched=(4, 5))  # a negative start, an end behind the clip
    assert nf.min() > 2
    assert_array_equal(got, want)
    assert (got[[1, 4, 5]] == FILL).all() and (got[[0, 2, 3], :, 0] > 0).all()
    got, _, want, _ = autocorr_given(clips[:3], crops[:3], 1102, 441, 12, ham, n_frames=[3, 0, 6], ld=6)
    assert_array_equal(got, want)
    assert (got[1] == FILL).all() and (got[0, 3:] == FILL).all()
    # max_len below the longest clip: that clip is left alone
    pcm, off = pack(clips[:3])
    se = np.asarray(crops[:3], np.int32)
    nf = np.array([P.frame_count(e - s, 1102, 441) for s, e in se], np.int32)
    dev = lambda a: torch.as_tensor(a).to("cuda")
    got, _ = autocorr_raw(dev(pcm), dev(off), 3, 3007, 1102, 441, 12, dev(ham), dev(se), dev(nf), dev(np.zeros(3, np.int32)), 0, 5)
    want = R.autocorr_batch(clips[:3], se, nf, [0, 0, 1], 1102, 441, 12, ham, 5, FILL)
    assert_array_equal(got, want)
    assert (got[2] == FILL).all()
    # every condition of the gate in one batch (crop_frame_cases.gate_batch), as separate arrays and as rows
    for stride in (0, 19):
        got, count, want, _ = autocorr_given(p=8, stride=stride, **C.gate_batch())
        assert_array_equal(got, want)
        assert (got[C.GATE_UNTOUCHED] == FILL).all() and (got[[0, 2], :, 0] > 0).all() and count == 0
        assert not got[8, 0].any() and (got[8, 1:] == FILL).all()  # the empty crop's one all-zero frame


def crafted_rows(p):
    """The CPU test's crafted rows padded to p + 1 entries, rows at and above 2^53, and random rows that
    stop at every order."""
    def pad(v):
        v = list(v)[:p + 1]
        return v + [0] * (p + 1 - len(v))

    rows = [pad(2 ** (40 - j) for j in range(33)), pad([1, 1, 1, 1, 1]), pad([1, 2, 0]), pad([-3, 1, 1]), pad([0]),
            pad([4, 2, 4, 0]), pad([8, 4, 2, 1]), pad([2 ** 53 + 1, 0]), pad([2 ** 53 + 3, 1]), pad([-(2 ** 53) - 1, 5]),
            pad([2 ** 60, 2 ** 53 + 1]), pad([2 ** 62 + 2 ** 9 + 1, 2 ** 61 + 3, 2 ** 60 - 1, -(2 ** 59) - 7]),
            pad([2 ** 63 - 1] * 3), pad([-(2 ** 63)] * 2), pad([5, -5]), pad([5, 5]), pad([7, -6, 5, -4, 3, -2, 1])]
    rng = np.random.default_rng(14)
    for j in range(40):  # a decaying random sequence: stops anywhere between order 0 and p
        mag = 10 ** rng.uniform(3, 15)
        rows.append(pad([int(mag)] + [int(v) for v in mag * rng.uniform(-1, 1, p) * 0.8 ** np.arange(1, p + 1) *
                                      rng.uniform(0.2, 1.3)]))
    return np.array(rows, np.int64)


@functools.lru_cache(maxsize=None)
def solve_pool(p):
    """Rows for dsp_lpc_solve at order p: the restatement's r of the test shapes (cut to p + 1 lags, which
    is r at order p) and the crafted rows -> int64 [m, p + 1]."""
    rows = [crafted_rows(p)]
    for L, S, window in ((1102, 441, "hamming"), (64, 16, "none"), (33, 7, "hanning")):
        if p <= L - 1:
            full = shape_reference(L, S, 32 if L == 33 else (12 if L == 1102 else 8), window)
            if full.shape[2] >= p + 1:
                rows.append(full[full[:, :, 0] != FILL][::7, :p + 1])
    return np.concatenate(rows)


@pytest.mark.parametrize("p,Q,n", ((1, 0, 1), (1, 5, 64), (1, 64, 65), (12, 12, 1000), (12, 5, 65), (12, 0, 64), (12, 64, 64),
                                   (32, 64, 65), (32, 12, 1000), (32, 5, 1), (32, 0, 64)))
def test_solve_against_the_restatement(p, Q, n):
    """Orders 1, 12, 32 with Q = 0, 5 (< p at 12 and 32), 12 and 64 (> p), n = 1, 64, 65 (one block, and one
    thread over) and 1000: frames' r and the crafted rows mixed in one launch, every stop order next to
    every other; bit patterns equal, no NaN anywhere."""
    pool = solve_pool(p)
    if n >= len(pool):
        pick = np.arange(n) % len(pool)
    else:  # half crafted rows (they come first), half frames
        pick = np.concatenate([np.arange(n // 2), np.linspace(57, len(pool) - 1, n - n // 2).astype(np.int64)])
    r = pool[np.random.default_rng(100 * p + Q).permutation(pick)]
    got = solve_raw(r, p, Q)
    want = R.solve(r, p, Q)
    same_solution(got, want)
    if n >= 64:
        assert len(set(want[3].tolist())) >= (2 if p == 1 else 3)  # mixed stop orders in the launch: 0, 1, p at least


def test_solve_known_answers():
    got = solve_raw([[2 ** (20 - j) for j in range(9)], [1, 1, 1, 1, 1, 0, 0, 0, 0], [1, 2, 0, 0, 0, 0, 0, 0, 0],
                     [-3, 1, 1, 0, 0, 0, 0, 0, 0], [0] * 9], 8, 4)
    a, k, err, reached, cep = got
    assert a[0].tolist() == [0.5] + [0.0] * 7 and cep[0].tolist() == [0.5, 0.125, 1.0 / 24.0, 0.015625]
    assert err.tolist() == [786432.0, 1.0, 1.0, -3.0, 0.0] and reached.tolist() == [8, 0, 0, 0, 0]
    assert not a[1:].any() and not k[1:].any() and not cep[1:].any()


def test_both_calls_in_a_graph():
    """dsp_lpc_autocorr and dsp_lpc_solve (no allocation, no sync) captured in a single-stream graph and
    replayed twice: the eager results."""
    import torch
    from src import _hip
    lib = _hip.lib()
    clips, crops = shape_clips(64)
    L, S, p, Q, B = 64, 16, 8, 12, len(clips)
    table = table_of("hamming", L)
    pcm, off = pack(clips, lead=3)
    se = np.asarray(crops, np.int32)
    nf = np.array([P.frame_count(e - s, L, S) for s, e in se], np.int32)
    status = np.zeros(B, np.int32)
    ld, max_len = int(nf.max()), max(len(c) for c in clips)
    want_r = R.autocorr_batch(clips, se, nf, status, L, S, p, table, ld, 0)
    want = R.solve(want_r, p, Q)
    t = [torch.as_tensor(a).to("cuda") for a in (pcm, off, se, nf, status, table)]
    r = torch.zeros((B, ld, p + 1), dtype=torch.int64, device="cuda")
    outs = [torch.empty(s, dtype=dt, device="cuda") for s, dt in (((B * ld, p), torch.float64), ((B * ld, p), torch.float64),
                                                                   ((B * ld,), torch.float64), ((B * ld,), torch.int32),
                                                                   ((B * ld, Q), torch.float64))]
    nbytes = lib.dsp_lpc_workspace_bytes(B, max_len, L, S, p)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def call():
        rc = lib.dsp_lpc_autocorr(_hip.ptr(t[0]), _hip.ptr(t[1]), B, max_len, L, S, p, _hip.ptr(t[5]), _hip.ptr(t[2]),
                                  _hip.ptr(t[3]), _hip.ptr(t[4]), 0, _hip.ptr(r), ld, _hip.ptr(ws), nbytes, _hip.stream_handle())
        assert rc == 0
        rc = lib.dsp_lpc_solve(_hip.ptr(r), B * ld, p, Q, *[_hip.ptr(o) for o in outs], _hip.stream_handle())
        assert rc == 0

    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        r.zero_()
        for o in outs:
            o.fill_(-5)
        ws.fill_(0x55)
        g.replay()
        torch.cuda.synchronize()
        assert_array_equal(r.cpu().numpy(), want_r)
        same_solution([o.cpu().numpy() for o in outs], want)
        assert int(ws[:4].view(torch.int32).item()) == 0


def analyzer_reference(clips, h, L, S, p, Q, window, ld):
    se, nf, status = h[:, 15:17], h[:, 17], h[:, 18]
    r = R.autocorr_batch(clips, se, nf, status, L, S, p, table_of(window, L), ld, 0)
    a, k, err, reached, cep = R.solve(r, p, Q)
    B = len(clips)
    return dict(r=r, a=a.reshape(B, ld, p), k=k.reshape(B, ld, p), err=err.reshape(B, ld), reached=reached.reshape(B, ld),
                cep=cep.reshape(B, ld, Q))


def same_analysis(res, want):
    assert_array_equal(res["r"], want["r"])
    assert_array_equal(res["reached"], want["reached"])
    for key in ("a", "k", "err", "cep"):
        assert res[key].shape == want[key].shape
        assert_array_equal(bits(res[key]), bits(want[key]), err_msg=key)


def test_lpc_analyzer():
    """LpcAnalyzer after a real extraction: a padded [B, N] batch and a packed batch with offsets and clips
    of different lengths; zeros behind each clip's frames."""
    import torch
    from src.pipeline import FeatureExtractor, LpcAnalyzer
    from src.synth import make_clip
    fx = FeatureExtractor(1102, 441, "hamming", True)
    padded = np.stack([make_clip(700 + j, n_samples=11025, label=j) for j in range(8)])
    pcm_t = torch.as_tensor(padded).to("cuda")
    out = fx(pcm_t)
    an = LpcAnalyzer(1102, 441)
    res = {k: v.cpu().numpy() for k, v in an(pcm_t, out).items()}
    h = out["rows"].cpu().numpy()
    ld = an.frames(11025)
    assert res["r"].shape == (8, ld, 13) and res["cep"].shape == (8, ld, 12) and an.plain_frames() == 0
    assert ((h[:, 18] & 0xFF) == 0).all() and h[:, 17].min() >= 1 and h[:, 17].max() <= ld
    want = analyzer_reference(list(padded), h, 1102, 441, 12, 12, "hamming", ld)
    same_analysis(res, want)
    inside = np.arange(ld)[None, :] < h[:, 17][:, None]
    assert not res["r"][~inside].any() and not res["cep"][~inside].any() and not res["err"][~inside].any()
    # packed, ragged, another order and window, Q > p
    clips = [make_clip(800 + j, n_samples=9000 + 1013 * j, label=j) for j in range(5)]
    pcm, off = pack(clips)
    pcm_t, max_len = torch.as_tensor(pcm).to("cuda"), max(len(c) for c in clips)
    out = fx(pcm_t, off, max_len=max_len)
    an = LpcAnalyzer(1102, 441, order=8, n_cep=10, window_type="rectangular")
    res = {k: v.cpu().numpy() for k, v in an(pcm_t, out, off, max_len=max_len).items()}
    h = out["rows"].cpu().numpy()
    want = analyzer_reference(clips, h, 1102, 441, 8, 10, "none", an.frames(max_len))
    same_analysis(res, want)
    with pytest.raises(ValueError):
        an(np.zeros((2, 4000), np.int32), {"rows": None})


def test_extract_both_with_lpc(tmp_path):
    """extract_both(lpc=6) on 3 x 4 WAV files, with and without pitch=True: the columns of the calls
    without it stay in front, bit for bit; the six cepstra are the last sequence columns (behind f0) and
    their means then standard deviations the last 12 matrix columns, equal to the restatement's (order 12)."""
    import torch
    from src.audio_processing import load_wav_pcm
    from src.dataset import PCMDataset
    from src.pipeline import FeatureExtractor
    C.wav_tree(tmp_path, 4, 4000)
    ds = PCMDataset(str(tmp_path))
    X15, y, seq2, lengths = ds.extract_both(1102, 441)
    X27, y2, seq8, lengths2 = ds.extract_both(1102, 441, lpc=6)
    X20, _, seq3, _ = ds.extract_both(1102, 441, pitch=True)
    X32, _, seq9, _ = ds.extract_both(1102, 441, pitch=True, lpc=6)
    assert X27.shape == (12, 27) and X32.shape == (12, 32) and seq8.shape == seq2.shape[:2] + (8,) and seq9.shape == seq2.shape[:2] + (9,)
    assert_array_equal(bits(X27[:, :15]), bits(X15))
    assert_array_equal(bits(X32[:, :20]), bits(X20))
    assert_array_equal(bits(seq8[:, :, :2]), bits(seq2))
    assert_array_equal(bits(seq9[:, :, :3]), bits(seq3))
    assert_array_equal(bits(seq9[:, :, 3:]), bits(seq8[:, :, 2:]))
    assert_array_equal(bits(X32[:, 20:]), bits(X27[:, 15:]))
    assert_array_equal(y, y2)
    assert_array_equal(lengths, lengths2)
    clips = [load_wav_pcm(f)[0] for f, _ in ds.files]
    pcm, off = pack(clips)
    fx = FeatureExtractor(1102, 441, "hamming", True)
    h = fx(torch.as_tensor(pcm).to("cuda"), off, max_len=int(np.diff(off).max()))["rows"].cpu().numpy()
    width = int(h[:, 17].max())
    want = analyzer_reference(clips, h, 1102, 441, 12, 6, "hamming", width)
    assert_array_equal(bits(seq8[:, :, 2:]), bits(want["cep"]))
    stats = np.stack([R.lpcc_stats(c, n) for c, n in zip(want["cep"], h[:, 17])])
    assert_array_equal(bits(X27[:, 15:]), bits(stats))
    assert (stats[:, 6:] > 0).all()
    # 16-bit stereo whose channel sums need int32: the analysis takes int16 only
    _write_wav(tmp_path / "w0" / "stereo.wav", np.repeat(np.random.default_rng(5).integers(-30000, 30000, (30000, 1)), 2, axis=1).astype(np.int16), channels=2)
    wide = PCMDataset(str(tmp_path))
    assert len(wide.parts) == 2
    with pytest.raises(ValueError):
        wide.extract_both(1102, 441, lpc=6)
    assert wide.extract_both(1102, 441)[0].shape[1] == 15


def test_compare_with_lpc(tmp_path):
    """compare(lpc=6, hmm=True): the rows of the table plus 'HMM', on the 27-d matrix and the 8-channel
    sequences; the KNN's statistical accuracy is the 3-NN's on extract_both(lpc=6)'s own matrix."""
    import compare_feature_methods as cfm
    from sklearn.model_selection import train_test_split
    from src.feature_extraction import normalize_features
    from src.models import create_classifier
    C.wav_tree(tmp_path, 5, 5000)
    res = cfm.compare(str(tmp_path), hmm=True, lpc=6)
    assert list(res) == ["KNN", "SVM", "Decision Tree", "HMM"]
    X27, X_seq, y, lengths = cfm.load_both_methods(str(tmp_path), lpc=6)
    assert X27.shape == (15, 27) and X_seq.shape[2] == 8
    tr, te, y_tr, y_te = train_test_split(X27, y, test_size=0.2, random_state=42, stratify=y)
    tr, m, sd = normalize_features(tr)
    te, _, _ = normalize_features(te, m, sd)
    want = float(create_classifier('knn', n_neighbors=3).fit(tr, y_tr).evaluate(te, y_te)['accuracy'])
    assert res["KNN"]["statistical"] == want == res["HMM"]["statistical"] and 0.0 <= res["HMM"]["sequence"] <= 1.0
    with pytest.raises(ValueError):
        cfm.compare(str(tmp_path), hmm=True, lpc=7)


def test_knn_on_cepstral_statistics_end_to_end():
    """300 labelled synthetic clips of 1 s: the 24 cepstral statistics of the device path are the
    restatement's bit for bit, so the 3-NN on their z-scores (80/20 stratified split, random_state 42)
    predicts the same labels and reaches the restatement's accuracy exactly."""
    import torch
    from sklearn.model_selection import train_test_split
    from src.feature_extraction import normalize_features
    from src.models import create_classifier
    from src.pipeline import FeatureExtractor, LpcAnalyzer, lpcc_statistics
    from src.synth import make_batch
    pcm, y = make_batch(300, base_seed=7, with_labels=True)
    pcm_t = torch.as_tensor(pcm).to("cuda")
    out = FeatureExtractor(1102, 441, "hamming", True)(pcm_t)
    an = LpcAnalyzer(1102, 441)
    res = {k: v.cpu().numpy() for k, v in an(pcm_t, out).items()}
    h = out["rows"].cpu().numpy()
    nf = h[:, 17]
    assert ((h[:, 18] & 0xFF) == 0).all()
    want = analyzer_reference(list(pcm), h, 1102, 441, 12, 12, "hamming", res["r"].shape[1])
    same_analysis(res, want)
    ref_stats = np.stack([R.lpcc_stats(c, n) for c, n in zip(want["cep"], nf)])
    dev_stats = lpcc_statistics(res["cep"], nf)
    assert_array_equal(bits(dev_stats), bits(ref_stats))

    def knn(X):
        tr, te, y_tr, y_te = train_test_split(X, y, test_size=0.2, random_state=42, stratify=y)
        tr, m, sd = normalize_features(tr)
        te, _, _ = normalize_features(te, m, sd)
        pred = np.asarray(create_classifier('knn', n_neighbors=3).fit(tr, y_tr).predict(te))
        return pred, float(np.mean(pred == y_te))

    (pred_d, acc_d), (pred_r, acc_r) = knn(dev_stats), knn(ref_stats)
    inside = np.arange(res["r"].shape[1])[None, :] < nf[:, None]
    print("3-NN on the 24 cepstral statistics: device %.4f, restatement %.4f; %d frames, %d stopped early, max |k| %.6f"
          % (acc_d, acc_r, inside.sum(), (res["reached"][inside] < 12).sum(), np.abs(res["k"]).max()))
    assert_array_equal(pred_d, pred_r)
    assert acc_d == acc_r
