"""The FAST extraction kernel's per-clip bookkeeping (extract_kernel<true>, csrc/extract.hip): the
persistent loop around a clip (the next clip's range, the 4-clip output chunk and its flush, the
clip queue and the static split), the small-crop and the general R5 statistics paths, and the clip
statistics that wave 0 broadcasts to the other waves (tpos, t0, nv, kneg).

Every launch is checked clip by clip against the C oracle with the project's tolerances (status,
start/end, n_frames exact; the 15-d vector through feat_close; per-frame E / M 1e-5 relative, ZCR
exact) and bit for bit against dsp_extract_general on the clips both kernels take.
"""
import numpy as np
import pytest

import edge_corpus as ec
import oracle
from test_gpu_extract import feat_close
from test_gpu_general import _general

pytestmark = pytest.mark.gpu

WINDOW = "hamming"
L0, S0 = 1102, 441
MAX_LEN = 6000      # the launches' explicit max_len: a longer clip is a bad clip (DSP_CLIP_TOO_LONG)
EMPTY, TOO_LONG = 1, 4
# ragged lengths in [2000, 6000], every residue mod 8 among them
POOL_LENS = (2000, 2337, 2790, 3123, 3604, 4093, 4502, 4999, 5394, 5731, 6000, 2049, 2455)
SHORT_LEN = 700     # shorter than a frame: no VAD frame, one zero-padded feature frame

_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _window(L):
    from src.pipeline import create_window
    return create_window(WINDOW, L)


def _pack(clips, lead):
    """Clips back to back after `lead` junk samples -> (pcm, offsets, each clip's lead)."""
    parts = [np.full(lead, 1234, np.int16)] + list(clips) + [np.zeros(16, np.int16)]
    off = np.zeros(len(clips) + 1, np.int64)
    off[0] = lead
    off[1:] = lead + np.cumsum([c.size for c in clips])
    return np.concatenate(parts), off, off[:-1] % 8


def _reference(clips, L, S, vad):
    """Oracle and dsp_extract_general results of a list of valid clips (computed once by the
    callers), the general kernel's checked against the oracle here."""
    w = _window(L)
    refs = [oracle.process_clip(c, L, S, w, do_vad=vad) for c in clips]
    pcm, off, _ = _pack(clips, 3)
    gen = _general(pcm, off, L, S, WINDOW, vad)
    for i, r in enumerate(refs):
        _check_clip(gen, i, r, ("general", i))
    return refs, gen


def _check_clip(out, i, r, what):
    assert (out["status"][i] & 0xFF) == r["status"], (what, out["status"][i], r["status"])
    if r["status"]:
        return
    assert tuple(out["start_end"][i]) == (r["start"], r["end"]), (what, out["start_end"][i], r["start"], r["end"])
    F = r["n_frames"]
    assert out["n_frames"][i] == F, (what, out["n_frames"][i], F)
    got = np.asarray(out["feat"][i], np.float64)
    assert np.isfinite(got).all(), (what, got)
    assert not feat_close(got, r["feat"]).any(), (what, got, r["feat"])
    if "seq" in out:
        seq = out["seq"][i, :F]
        np.testing.assert_array_equal(seq[:, 2], r["seq"][:, 2], err_msg=str(what))
        np.testing.assert_allclose(seq[:, 0], r["seq"][:, 0], rtol=1e-5, atol=1e-30, err_msg=str(what))
        np.testing.assert_allclose(seq[:, 1], r["seq"][:, 1], rtol=1e-5, atol=1e-30, err_msg=str(what))


def _same_bits(a, ia, b, ib, what):
    assert np.array_equal(_bits(a["feat"][ia]), _bits(b["feat"][ib])), (what, "feat", a["feat"][ia], b["feat"][ib])
    assert np.array_equal(a["start_end"][ia], b["start_end"][ib]), (what, "start_end")
    assert a["n_frames"][ia] == b["n_frames"][ib], (what, "n_frames")
    assert (a["status"][ia] & 0xFF) == (b["status"][ib] & 0xFF), (what, "status")
    if "seq" in a and "seq" in b:
        F = int(a["n_frames"][ia])
        assert np.array_equal(_bits(a["seq"][ia, :F]), _bits(b["seq"][ib, :F])), (what, "seq")


def _check_bad(out, i, status, what):
    assert (out["status"][i] & 0xFF) == status, (what, out["status"][i])
    assert np.isnan(out["feat"][i]).all(), (what, out["feat"][i])
    assert tuple(out["start_end"][i]) == (0, 0) and out["n_frames"][i] == 0, what


def _pool():
    """The valid clips of the loop tests (speech-like, ragged, + one shorter than a frame) with
    their oracle and general-kernel results."""
    if "pool" not in _CACHE:
        from src.synth import make_clip
        clips = [make_clip(4200 + k, n) for k, n in enumerate(POOL_LENS)] + [make_clip(4300, SHORT_LEN)]
        assert sorted(set(n % 8 for n in POOL_LENS)) == list(range(8))
        refs, gen = _reference(clips, L0, S0, True)
        assert refs[-1]["n_frames"] == 1 and len(refs[-1]["vad_energy"]) == 0
        _CACHE["pool"] = (clips, refs, gen)
    return _CACHE["pool"]


def _extractor():
    if "fx" not in _CACHE:
        from src.pipeline import FeatureExtractor
        assert ec.fast_layout(MAX_LEN, L0, S0) == 1
        _CACHE["fx"] = FeatureExtractor(L0, S0, WINDOW, True)
    return _CACHE["fx"]


def _launch_twice(fx, pcm, off, max_len):
    """The same launch twice on one extractor (its queue scratch and output buffers are reused)."""
    import torch
    t = torch.as_tensor(pcm).cuda()
    outs = []
    for _ in range(2):
        out = fx(t, off, max_len=max_len)
        outs.append({k: v.cpu().numpy().copy() for k, v in out.items() if k != "rows"})
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), ("second launch", k)
    return outs[1]


def _build(src):
    """src: per clip a pool index, or "empty" / "bad" -> the clips of a launch."""
    from src.synth import make_clip
    clips, _, _ = _pool()
    bad = make_clip(4400, MAX_LEN + 100)
    return [np.zeros(0, np.int16) if s == "empty" else bad if s == "bad" else clips[s] for s in src]


def _check_launch(out, src, what):
    _, refs, gen = _pool()
    for i, s in enumerate(src):
        if s == "empty":
            _check_bad(out, i, EMPTY, what + (i,))
        elif s == "bad":
            _check_bad(out, i, TOO_LONG, what + (i,))
        else:
            _check_clip(out, i, refs[s], what + (i, s))
            _same_bits(out, i, gen, s, what + (i, s, "vs general"))


SHORT = len(POOL_LENS)  # the pool index of the too-short clip


def test_small_launches_straddle_the_output_chunk():
    """1, 3, 4, 5 and 9 clips (each workgroup one clip, chunks of 4 staged outputs), with an empty
    clip, a clip shorter than a frame and a too-long clip at the first, a middle and the last place of
    a chunk in turn; ragged lengths, so that the clips' leads cover 0-7."""
    fx = _extractor()
    leads, n = set(), 0
    for B in (1, 3, 4, 5, 9):
        last = min(B, 4) - 1  # the last place of the first chunk that this launch has
        mid = 1 if last > 1 else None
        for rot in range(3):
            kinds = ["empty", SHORT, "bad"]
            kinds = kinds[rot:] + kinds[:rot]
            src = [(7 * B + 3 * rot + i) % len(POOL_LENS) for i in range(B)]
            places = [0] if B == 1 else [0, last] if mid is None else [0, mid, last]
            for pl, kd in zip(places, kinds):
                src[pl] = kd
            if B == 9:  # the third chunk holds one clip: special as well
                src[8] = kinds[0]
            pcm, off, ld = _pack(_build(src), (B + rot) % 8)
            leads.update(int(x) for x in ld)
            out = _launch_twice(fx, pcm, off, MAX_LEN)
            _check_launch(out, src, ("small", B, rot))
            n += 1
    assert leads == set(range(8)) and n == 15


def _grid():
    import torch
    return 3 * torch.cuda.get_device_properties(0).multi_processor_count  # EXTRACT_WG_PER_CU workgroups per CU


def _big_launch(B, tag, pool_idx):
    """B clips cycling through pool_idx, with an empty, a short and a bad clip at the first, middle
    and last place of some chunks; every row against its source clip's reference, vectorised."""
    fx = _extractor()
    _, refs, gen = _pool()
    src = [pool_idx[i % len(pool_idx)] for i in range(B)]
    for c0, kinds in ((0, ("empty", SHORT, "bad")), (4 * (B // 8), ("bad", "empty", SHORT)),
                      (4 * ((B - 4) // 4), (SHORT, "bad", "empty"))):
        for pl, kd in zip((0, 2, 3), kinds):
            src[c0 + pl] = kd
    pcm, off, ld = _pack(_build(src), 5)
    assert set(int(x) for x in ld) == set(range(8))
    out = _launch_twice(fx, pcm, off, MAX_LEN)
    feat = _bits(out["feat"])
    seen = set()
    for s in set(src):
        rows = np.array([i for i, x in enumerate(src) if x == s])
        if s in ("empty", "bad"):
            for i in rows:
                _check_bad(out, i, EMPTY if s == "empty" else TOO_LONG, (tag, i))
            continue
        _check_clip(out, rows[0], refs[s], (tag, s))
        assert (feat[rows] == _bits(gen["feat"][s])).all(), (tag, s, "feat bits")
        assert (out["start_end"][rows] == gen["start_end"][s]).all(), (tag, s)
        assert (out["n_frames"][rows] == gen["n_frames"][s]).all(), (tag, s)
        assert ((out["status"][rows] & 0xFF) == 0).all(), (tag, s)
        seen.add(s)
    assert seen == set(pool_idx) | {SHORT}


def test_static_split_with_second_clips():
    """More clips than workgroups, at most 1.5 per workgroup: the static split (clip i, then i + G)."""
    G = _grid()
    B = G + G // 3
    assert B > G and 2 * B <= 3 * G
    _big_launch(B, "static", list(range(len(POOL_LENS))))


def test_claimed_queue_chunks_of_two():
    """More than two clips per workgroup: claimed chunks of two clips (half an output chunk)."""
    G = _grid()
    B = 2 * G + 37
    assert 2 * G < B < 64 * G
    _big_launch(B, "queue2", list(range(len(POOL_LENS))))


def test_claimed_queue_chunks_of_four():
    """64 clips per workgroup and more: claimed chunks of four clips, each staged and flushed whole
    (the pool's shorter clips only, to keep the batch small)."""
    G = _grid()
    short_idx = [k for k, n in enumerate(POOL_LENS) if n < 2800]
    assert len(short_idx) == 5  # (coprime to the chunk: a clip takes every place of a chunk)
    _big_launch(64 * G + 3, "queue4", short_idx)


# ---- R5 paths ------------------------------------------------------------------------------
R5_L, R5_S = 64, 32
R5_FRAMES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128)


def _r5_clips():
    from src.synth import make_clip
    out = []
    for F in R5_FRAMES:
        n = R5_L + (F - 1) * R5_S
        out.append(("F%d_speech" % F, F, make_clip(5100 + F, n)))
        # period 16 divides the shift: every frame holds the same samples -> all of E, M, ZCR tie
        tied = np.round(9000 * np.sin(2 * np.pi * (np.arange(n) + 0.25) / 16)).astype(np.int16)
        out.append(("F%d_tied" % F, F, tied))
        x = tied.copy()  # one frame in three a little louder: groups of ties around the median
        for f in range(0, F, 3):
            x[f * R5_S + R5_L // 2] += 40
        out.append(("F%d_tied_groups" % F, F, x))
        if F > 1:  # the last frame zero-padded (one sample past the frame before it)
            out.append(("F%d_padded" % F, F, make_clip(5300 + F, R5_L + (F - 2) * R5_S + 1)))
    return out


def test_r5_paths_frame_counts_and_ties():
    """Endpoint detection off: 1, 2, 31, 32, 33 (the small-crop jobs and the first count past them),
    63, 64, 65, 127 and 128 feature frames at a 64 / 32 frame, with ordinary, all-equal and
    partly-equal sequences."""
    import torch
    from src.pipeline import FeatureExtractor
    named = _r5_clips()
    clips = [c for _, _, c in named]
    longest = max(c.size for c in clips)
    assert ec.fast_layout(longest, R5_L, R5_S) == 1
    refs, gen = _reference(clips, R5_L, R5_S, False)
    for (name, F, _), r in zip(named, refs):
        assert r["status"] == 0 and r["n_frames"] == F, (name, r["n_frames"])
    fx = FeatureExtractor(R5_L, R5_S, WINDOW, False, return_sequences=True)
    for lead in (0, 3, 6):
        pcm, off, _ = _pack(clips, lead)
        out = {k: v.cpu().numpy().copy() for k, v in fx(torch.as_tensor(pcm).cuda(), off).items()}
        for i, ((name, F, _), r) in enumerate(zip(named, refs)):
            _check_clip(out, i, r, ("r5", lead, name))
            _same_bits(out, i, gen, i, ("r5", lead, name, "vs general"))


# ---- statistics broadcast ------------------------------------------------------------------
def _dc_clip(seed, n, dc, frac=0):
    """A clip whose mean is exactly dc + frac / 4 (n a multiple of 8): antisymmetric noise, whose sum
    is 0, + dc, and + 1 on the first frac quarters of the clip."""
    rng = np.random.default_rng(seed)
    h = rng.integers(-9000, 9001, n // 2)
    h[n // 8:n // 4] //= 30  # a quiet stretch, so that the endpoints are not the clip's ends
    x = np.concatenate([h, -h[::-1]]).astype(np.int64) + dc
    x[:frac * (n // 4)] += 1
    assert x.min() >= -32768 and x.max() <= 32767
    return x.astype(np.int16)


@pytest.mark.parametrize("vad", [True, False], ids=["vad", "novad"])
def test_statistics_broadcast_dc_offsets(vad):
    """Clips whose rounded mean t0 is -3, -2, 0, 2, 3 and 20000 (both branches of the near-zero
    centring, either sign), with means on and off the integers (t0 == tpos or tpos - 1), and one
    clip holding a -32768 sample (kneg)."""
    import torch
    from src.pipeline import FeatureExtractor
    n = 5200
    named = []
    for dc in (-3, -2, 0, 2, 3, 20000):
        for frac in (0, 1, 3):  # mean dc, dc + 1/4 (t0 = dc = tpos - 1), dc + 3/4 (t0 = dc + 1 = tpos)
            if frac == 3:
                c = _dc_clip(6000 + dc % 97, n, dc - 1, 3)
            else:
                c = _dc_clip(6100 + dc % 97 + frac, n, dc, frac)
            mean = c.astype(np.float64).mean()
            assert int(np.floor(mean + 0.5)) == dc, (dc, frac, mean)
            named.append(("dc%d_q%d" % (dc, frac), c))
    neg = _dc_clip(6200, n, -9000)
    neg[1777] = -32768
    named.append(("kneg", neg))
    clips = [c for _, c in named]
    refs, gen = _reference(clips, L0, S0, vad)
    fx = FeatureExtractor(L0, S0, WINDOW, vad, return_sequences=True)
    assert ec.fast_layout(n, L0, S0) == 1
    for lead in (0, 5):
        pcm, off, _ = _pack(clips, lead)
        out = {k: v.cpu().numpy().copy() for k, v in fx(torch.as_tensor(pcm).cuda(), off).items()}
        for i, ((name, _), r) in enumerate(zip(named, refs)):
            assert r["status"] == 0, name
            _check_clip(out, i, r, ("stats", vad, lead, name))
            _same_bits(out, i, gen, i, ("stats", vad, lead, name, "vs general"))
