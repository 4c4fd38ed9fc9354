"""The jobs that clip_fast (csrc/extract.hip) gives to its last wave: the ZCR of every crop frame
(crop_zcr, a lane per frame, before any R4 rows that wave holds) and the next clip's hand-over
(sh->noff) -- and with them the FAST loop's step from one clip to the next.

Frame counts around the two hand-over points of the ZCR wave (28 / 29: the last wave starts to
hold R4 rows; 64 / 65: its lane loop wraps), and next-clip patterns of the shortest and the longest
FAST clip.  Every result is checked against the C oracle (status, start/end, n_frames, the ZCR
column exact; feat and the E / M columns 1e-5) and bit for bit against dsp_extract_general, never
against the fused kernel alone.
"""
import numpy as np
import pytest

import edge_corpus as ec
from test_gpu_clip_loop import EMPTY, TOO_LONG, _bits, _check_bad, _check_clip, _pack, _reference, _same_bits

pytestmark = pytest.mark.gpu

WINDOW = "hamming"
L0, S0 = 1102, 441
FRAMES = (1, 27, 28, 29, 63, 64, 65, 98)
SEED0 = 7100  # make_clip seeds SEED0 + 2 F + twin: with the VAD on, crops on both sides of 28 frames

_CACHE = {}


def _np(out):
    return {k: v.cpu().numpy().copy() for k, v in out.items() if k != "rows"}


def _frame_clips():
    """(name, F, clip): n = L + (F - 1) S, and for F > 1 the twin whose last frame is zero padded."""
    from src.synth import make_clip
    named = []
    for F in FRAMES:
        named.append(("F%d" % F, F, make_clip(SEED0 + 2 * F, L0 + (F - 1) * S0)))
        if F > 1:
            named.append(("F%d_padded" % F, F, make_clip(SEED0 + 2 * F + 1, L0 + (F - 2) * S0 + 1)))
    return named


def _frame_refs(vad):
    key = ("frames", vad)
    if key not in _CACHE:
        named = _frame_clips()
        clips = [c for _, _, c in named]
        assert ec.fast_layout(max(c.size for c in clips), L0, S0) == 1
        refs, gen = _reference(clips, L0, S0, vad)
        _CACHE[key] = (named, clips, refs, gen)
    return _CACHE[key]


def _run_leads(vad):
    import torch
    from src.pipeline import FeatureExtractor
    named, clips, refs, gen = _frame_refs(vad)
    fx = FeatureExtractor(L0, S0, WINDOW, vad, return_sequences=True)
    leads = set()
    for lead in range(8):
        pcm, off, ld = _pack(clips, lead)
        leads.update(int(x) for x in ld)
        out = _np(fx(torch.as_tensor(pcm).cuda(), off))
        for i, ((name, _, _), r) in enumerate(zip(named, refs)):
            _check_clip(out, i, r, ("frames", vad, lead, name))  # n_frames and the ZCR column exact, feat 1e-5
            _same_bits(out, i, gen, i, ("frames", vad, lead, name, "vs general"))
    assert leads == set(range(8))


def test_frame_counts_around_the_zcr_wave_hand_overs():
    """Endpoint detection off, so the length fixes F: 1, 27, 28, 29 (the last wave's first rows), 63,
    64, 65 (the ZCR lane loop's second pass) and 98 frames, each with its zero-padded twin, packed
    back to back at leads 0-7."""
    named, _, refs, _ = _frame_refs(False)
    for (name, F, _), r in zip(named, refs):
        assert r["status"] == 0 and r["n_frames"] == F, (name, r["n_frames"])
    _run_leads(False)


def test_vad_crops_on_both_sides_of_the_last_waves_rows():
    """The same clips with the VAD on: the oracle's crops (computed on the CPU) lie on both sides of
    28 frames, where the last wave holds no rows / its first rows."""
    _, _, refs, _ = _frame_refs(True)
    nf = [r["n_frames"] for r in refs]
    assert all(r["status"] == 0 for r in refs)
    assert min(nf) <= 28 < max(nf), nf
    _run_leads(True)


# ---- next-clip patterns ----------------------------------------------------------------------
def _pair():
    """The shortest clip (n = L) and the longest FAST clip, their oracle / general results, and
    their rows extracted one per call (a launch of one clip has no next clip)."""
    if "pair" not in _CACHE:
        import torch
        from src.pipeline import FeatureExtractor
        from src.synth import make_clip
        cap = ec.fast_cap(L0, S0)
        assert cap > 40000 and ec.fast_layout(cap, L0, S0) == 1 and ec.fast_layout(cap + 1, L0, S0) == 0
        clips = [make_clip(7501, L0), make_clip(7502, cap)]
        refs, gen = _reference(clips, L0, S0, True)
        fx = FeatureExtractor(L0, S0, WINDOW, True, return_sequences=True)
        single = []
        for i, c in enumerate(clips):  # the one-clip batch
            pcm, off, _ = _pack([c], 0)
            out = _np(fx(torch.as_tensor(pcm).cuda(), off, max_len=cap))
            _check_clip(out, 0, refs[i], ("single", i))
            _same_bits(out, 0, gen, i, ("single", i, "vs general"))
            single.append(out)
        _CACHE["pair"] = (cap, clips, refs, gen, single, fx)
    return _CACHE["pair"]


def _expect_rows(out, idx, single, what):
    """Rows idx of a launch (numpy arrays) against the one-clip launch `single`, bit for bit."""
    assert (_bits(out["feat"][idx]) == _bits(single["feat"][0])).all(), (what, "feat")
    assert (out["start_end"][idx] == single["start_end"][0]).all(), (what, "start_end")
    assert (out["n_frames"][idx] == single["n_frames"][0]).all(), (what, "n_frames")
    assert (out["status"][idx] == single["status"][0]).all(), (what, "status")
    F = int(single["n_frames"][0])
    assert (_bits(out["seq"][idx, :F]) == _bits(single["seq"][0, :F])).all(), (what, "seq")


def _grid():
    import torch
    return 3 * torch.cuda.get_device_properties(0).multi_processor_count  # EXTRACT_WG_PER_CU workgroups per CU


def _alternating(B, lead=0):
    """B clips, short / long in turn, built on the device -> (pcm tensor, offsets)."""
    import torch
    cap, clips, _, _, _, _ = _pair()
    two = torch.as_tensor(np.concatenate(clips)).cuda()
    parts = [torch.full((lead,), 1234, dtype=torch.int16, device="cuda"), two.repeat(B // 2)]
    if B & 1:
        parts.append(two[:L0])
    parts.append(torch.zeros(16, dtype=torch.int16, device="cuda"))
    lens = np.where(np.arange(B) % 2 == 0, L0, cap)
    off = np.concatenate([[lead], lead + np.cumsum(lens)]).astype(np.int64)
    return torch.cat(parts), off


@pytest.mark.parametrize("kind", ["static", "queue1", "queue2", "queue4"])
def test_alternating_shortest_and_longest_clip(kind):
    """The static split, claimed chunks of one, two and four clips (with their guided tails), as
    test_gpu_clip_loop sizes them; rows against the clips extracted one per call."""
    G = _grid()
    B = {"static": G + G // 3, "queue1": 2 * G - 5, "queue2": 2 * G + 37, "queue4": 64 * G + 3}[kind]
    assert {"static": 2 * B <= 3 * G, "queue1": 3 * G < 2 * B <= 4 * G, "queue2": 2 * G < B < 64 * G,
            "queue4": B >= 64 * G}[kind]
    cap, _, _, _, single, fx = _pair()
    pcm, off = _alternating(B, lead=3)
    out = _np(fx(pcm, off, max_len=cap))
    _expect_rows(out, np.arange(0, B, 2), single[0], (kind, "short"))
    _expect_rows(out, np.arange(1, B, 2), single[1], (kind, "long"))


def test_invalid_clip_between_valid_ones():
    """valid, invalid, valid: the invalid next clip is not touched and reports its status; the clips
    around it are the one-clip launches' bit for bit.  Both kinds of invalid clip, both orders."""
    import torch
    from src.synth import make_clip
    cap, clips, _, _, single, fx = _pair()
    bad = {"empty": (np.zeros(0, np.int16), EMPTY), "long": (make_clip(7503, cap + 1), TOO_LONG)}
    for name, (b, status) in bad.items():
        for a, z in ((0, 1), (1, 0)):
            pcm, off, _ = _pack([clips[a], b, clips[z]], 5)
            out = _np(fx(torch.as_tensor(pcm).cuda(), off, max_len=cap))
            _expect_rows(out, np.array([0]), single[a], (name, a, z, "first"))
            _check_bad(out, 1, status, (name, a, z))
            _expect_rows(out, np.array([2]), single[z], (name, a, z, "last"))


def test_last_clip_at_the_end_of_the_buffer():
    """The last clip ends where the caller's buffer ends (INTEGRATION.md's extract(): the clips back
    to back, no padding behind them)."""
    import torch
    cap, clips, _, _, single, fx = _pair()
    for order in ((0, 1), (1, 0), (1, 1)):
        cl = [clips[k] for k in order]
        pcm = torch.as_tensor(np.concatenate(cl)).cuda()
        off = np.concatenate([[0], np.cumsum([c.size for c in cl])]).astype(np.int64)
        assert off[-1] == pcm.numel()
        out = _np(fx(pcm, off, max_len=cap))
        for i, k in enumerate(order):
            _expect_rows(out, np.array([i]), single[k], ("unpadded", order, i))


def test_two_step_graph_replayed_twice():
    """Two launches of dsp_extract_features captured into one graph (ragged batches, their offsets
    on the device), replayed twice, against eager launches through FeatureExtractor."""
    import torch
    from src import _hip
    from src.pipeline import FeatureExtractor
    cap, _, _, _, single, fx = _pair()
    ld = (cap - L0 + S0 - 1) // S0 + 1
    hi, lo, zr = fx.ratios
    batches = []
    for B in (9, 14):
        pcm, off = _alternating(B, lead=B % 8)
        batches.append((pcm, off, torch.as_tensor(off).cuda(), torch.zeros(B, 19, dtype=torch.int32, device="cuda"),
                        torch.zeros(B, ld, 3, dtype=torch.float32, device="cuda")))
    cs = torch.cuda.Stream()
    queue = torch.zeros(_hip.QUEUE_WS_BYTES // 4, dtype=torch.int32, device="cuda")  # the capture stream's own

    def step(pcm, offd, rows, seq):
        r = rows.data_ptr()
        rc = _hip.lib().dsp_extract_features(
            _hip.ptr(pcm), _hip.ptr(offd), rows.shape[0], cap, L0, S0, _hip.ptr(fx.window), 1, hi, lo, zr,
            r, r + 60, r + 68, r + 72, 19, None, None, 0, _hip.ptr(seq), ld, _hip.ptr(queue), cs.cuda_stream)
        assert rc == 0, rc

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        for pcm, _, offd, rows, seq in batches:
            step(pcm, offd, rows, seq)
    for rep in range(2):
        for _, _, _, rows, seq in batches:
            rows.zero_()
            seq.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for pcm, off, _, rows, seq in batches:
            B = rows.shape[0]
            ref = _np(fx(pcm, off, max_len=cap))
            got = {"feat": rows[:, :15].contiguous().view(torch.float32).cpu().numpy(),
                   "start_end": rows[:, 15:17].cpu().numpy(), "n_frames": rows[:, 17].cpu().numpy(),
                   "status": rows[:, 18].cpu().numpy(), "seq": seq.cpu().numpy()}
            for k in ("feat", "start_end", "n_frames", "status"):
                assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(ref[k]).tobytes(), (rep, B, k)
            for i in range(B):
                F = int(ref["n_frames"][i])
                assert got["seq"][i, :F].tobytes() == ref["seq"][i, :F].tobytes(), (rep, B, i, "seq")
            _expect_rows(got, np.arange(0, B, 2), single[0], ("graph", rep, B, "short"))
            _expect_rows(got, np.arange(1, B, 2), single[1], ("graph", rep, B, "long"))
