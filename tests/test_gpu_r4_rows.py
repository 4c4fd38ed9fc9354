"""The crop frames' windowed E and M (r4_frames / frame_vec in csrc/extract.hip, canon_pair in
csrc/dsp_device.h): every variant of the row loop and the row bookkeeping around it.

The row loop runs a batch of up to R4_KV = 9 vectors per lane (144 vectors, 1152 samples per row) in
one of six forms: padded (the crop's last, zero-padded frame) or not, near0 (|round(mean)| <= 2: one
centring add) or not (two), and, for an unpadded frame, a batch every lane fills or one with
per-vector lane bounds.
  * L = 1260 / S = 441 (the longest frame of the FAST layout): 158-159 vectors per frame, the first
    batch full and a second, partial one at the 144-vector stride.
  * L = 1102 / S = 441: 138-139 vectors per frame, one batch, some lanes with 8 vectors.
  * L = 200 / S = 80: 25-26 vectors per frame, a batch is never full.
Clips: a speech-like clip about zero (near0) and its reverse on a DC offset of 1000 (not near0), at lengths
that give a crop of one whole frame, one short frame (m < L), five frames, five frames with the last
zero padded, 30 frames (rows on the last wave too) and 31 with a short last frame.  Each batch is
packed at leads 0-7; its first clip's length is 5 mod 8, so that at lead 3 it has an odd lead and ends
on a 16-byte boundary (the vfix patch of its last sample).

Each clip is checked against the C oracle (_check_clip: the tolerances of the other extraction
tests), and the FAST launch bit for bit against the generic layout (extract_kernel<false>) and
against dsp_extract_general.  With endpoint detection on, no clip may sit within the kernel's
certification margin: the oracle's energies are held against both thresholds at 1e-9, a hundred
times the kernel's 1e-11, on the CPU before any launch, and no result may carry the redo bit.
"""
import numpy as np
import pytest

import edge_corpus as ec
from test_gpu_clip_loop import _check_clip, _pack, _reference, _same_bits

pytestmark = pytest.mark.gpu

WINDOW = "hamming"
SIZES = {"1260_441": (1260, 441), "1102_441": (1102, 441), "200_80": (200, 80)}
DC = 1000
HI, LO = 0.5, 0.1  # FeatureExtractor's energy_high_ratio / energy_low_ratio
CASES = [(s, vad) for s in SIZES for vad in (False, True)]
_CACHE = {}


def _clips(L, S):
    """(name, clip, F with endpoint detection off).  The first clip of each kind has n = 5 mod 8."""
    from src.synth import make_clip
    n_fix = L + 2 * S
    n_fix += (5 - n_fix) % 8
    lens = [("vfix", n_fix, 3 + (n_fix > L + 2 * S)), ("one_frame", L, 1), ("short_frame", L - 37, 1),
            ("five", L + 4 * S, 5), ("five_padded", L + 3 * S + S // 2 + 3, 5), ("thirty", L + 29 * S, 30),
            ("thirty_one_padded", L + 29 * S + 5, 31)]
    named = []
    for k, (name, n, F) in enumerate(lens):
        x = make_clip(8100 + 10 * k + (L < 1000) + 2 * (L > 1200), n).astype(np.int64)
        x -= int(np.floor(x.mean() + 0.5))  # speech-like clips carry a small offset of their own
        for tag, y in (("_near0", x), ("_dc", np.clip(x[::-1] + DC, -32768, 32767))):
            t0 = int(np.floor(y.mean() + 0.5))
            assert abs(t0) <= 2 if tag == "_near0" else abs(t0 - DC) <= 50, (name, tag, y.mean())
            named.append((name + tag, np.ascontiguousarray(y.astype(np.int16)), F))
    return named  # the two vfix clips lead the batch: the first meets the case at lead 3, the second at 6


def _outside_margin(r, what):
    """The oracle's endpoint decisions against the certification margin (near_tie in dsp_device.h)
    at a hundred times the kernel's width: every VAD frame against the high threshold, and every
    frame before the first / after the last high-energy frame against the low one (the scan holds
    no other frame against it)."""
    E = np.asarray(r["vad_energy"], np.float64)
    nv = E.size
    if nv == 0:
        return
    nfr = min(5, nv // 10)
    noise = np.concatenate([E[:nfr], E[-nfr:]]).mean() if nfr else E.min()
    p90 = np.percentile(E, 90)
    t1, t2 = p90 * HI, noise + (p90 - noise) * LO

    def clear(e, t):
        return (np.abs(e - t) > 1e-9 * np.maximum(np.abs(e), abs(t))).all()

    assert clear(E, t1), (what, "high", t1)
    hi = np.nonzero(E > t1)[0]
    if hi.size:
        assert clear(np.concatenate([E[:hi[0]], E[hi[-1] + 1:]]), t2), (what, "low", t2)


def _refs(size, vad):
    key = (size, vad)
    if key not in _CACHE:
        L, S = SIZES[size]
        named = _clips(L, S)
        clips = [c for _, c, _ in named]
        refs, gen = _reference(clips, L, S, vad)
        for (name, _, F), r in zip(named, refs):
            assert r["status"] == 0, (size, vad, name, r["status"])
            if vad:
                _outside_margin(r, (size, name))
            else:
                assert r["n_frames"] == F, (size, name, r["n_frames"], F)
        _CACHE[key] = (named, clips, refs, gen)
    return _CACHE[key]


def _np(out):
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


@pytest.mark.parametrize("size,vad", CASES, ids=["%s-%s" % (s, "vad" if v else "novad") for s, v in CASES])
def test_row_loop_variants_on_every_path(size, vad):
    import torch
    from src.pipeline import FeatureExtractor
    L, S = SIZES[size]
    named, clips, refs, gen = _refs(size, vad)
    nf = [r["n_frames"] for r in refs]
    assert min(nf) == 1, nf  # a crop of one row
    if vad:  # crops that start inside the clip
        assert any(r["start"] > 0 for r in refs), [r["start"] for r in refs]
    else:  # the whole clip: rows on the last wave too
        assert max(nf) >= 29, nf
    longest = max(c.size for c in clips)
    assert ec.fast_layout(longest, L, S) == 1
    fx = FeatureExtractor(L, S, WINDOW, vad, return_sequences=True)
    fast0, seen, vfix = None, set(), 0
    for lead in range(8):
        pcm, off, ld = _pack(clips, lead)
        seen.update(int(x) for x in ld)
        vfix += sum(1 for c, a in zip(clips, ld) if (a & 1) and (a + c.size) % 8 == 0)
        out = _np(fx(torch.as_tensor(pcm).cuda(), off))
        assert not (out["status"] & 0x100).any(), (size, vad, lead, "a clip was redone as a near tie")
        for i, ((name, _, _), r) in enumerate(zip(named, refs)):
            _check_clip(out, i, r, (size, vad, "fast", lead, name))
            _same_bits(out, i, gen, i, (size, vad, "fast", lead, name, "vs general"))
        fast0 = fast0 or out
    assert seen == set(range(8)) and vfix >= 2, (seen, vfix)  # both leading clips met the vfix case
    # the generic layout: the same launch under a max_len the compile-time layout cannot hold
    max_len = max(longest, ec.fast_cap(L, S) + 1)
    assert max_len <= fx.fused_cap() and ec.fast_layout(max_len, L, S) == 0
    for lead in (0, 3):
        pcm, off, _ = _pack(clips, lead)
        out = _np(fx(torch.as_tensor(pcm).cuda(), off, max_len=max_len))
        for i, ((name, _, _), r) in enumerate(zip(named, refs)):
            _check_clip(out, i, r, (size, vad, "generic", lead, name))
            _same_bits(out, i, fast0, i, (size, vad, "generic", lead, name, "vs fast"))
            _same_bits(out, i, gen, i, (size, vad, "generic", lead, name, "vs general"))
