"""Pass A of the FAST extraction kernel (the exact moments of the VAD frames: whole-word totals
minus the half-word sums at the two frame ends) on the corpus of tests/vad_frame_end_cases.py, which
tests/test_vad_frame_ends_host.py pins on the CPU: every element of a word as a frame start and as a
frame end, at leads 0-7; -32768 runs in the kept and the dropped part of the half-words and across
the boundary; frame ends in the clip's first and last word; frames inside one word (L = 20, L = 2 --
the FAST layout does not refuse short frames, and L = 2 is the shortest frame that can also span two
words).

Every launch takes the FAST layout (dsp_extract_fast_layout == 1).  Per clip against the C oracle, as
test_gpu_edge_paths: status, start / end, n_frames, per-frame ZCR and VAD ZCR exact, VAD energies
1e-12 relative, per-frame E / M 1e-5 relative, the 15-d vector through feat_close; across the eight
leads every output is bit-identical.  No clip is skipped: the host test asserts oracle status 0 for
all of them.
"""
import numpy as np
import pytest

import edge_corpus as ec
import oracle
import vad_frame_end_cases as fc
from test_gpu_edge_paths import _check_launch, _same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", list(fc.GROUPS))
def test_frame_ends_vs_oracle(group):
    import torch
    from src.pipeline import FeatureExtractor, create_window
    L, S = fc.GROUPS[group]
    clips = fc.group_clips(group)
    assert clips and all(c.status == 0 for c in clips)
    w = create_window(fc.WINDOW, L)
    refs = {c.name: oracle.process_clip(c.pcm, L, S, w, do_vad=True) for c in clips}
    longest = max(c.pcm.size for c in clips)
    assert ec.fast_layout(longest, L, S) == 1, (group, longest)
    fx = FeatureExtractor(L, S, fc.WINDOW, True, return_vad_lists=True, return_sequences=True)
    tally = dict(abs_cells=0, cells=0)
    base = None
    for lead in fc.LEADS:
        pcm, off = ec.pack(clips, lead)
        out = {k: v.cpu().numpy().copy() for k, v in fx(torch.as_tensor(pcm).cuda(), off).items()}
        tag = (group, "vad", "fast", lead)
        _check_launch(out, clips, refs, True, tag, tally)
        if base is None:
            base = out
            continue
        for i, c in enumerate(clips):
            r = refs[c.name]
            what = tag + (c.name, "vs lead 0")
            _same_bits(base, i, out, i, r["n_frames"], what)
            nv = len(r["vad_energy"])
            assert np.array_equal(base["vad_energy"][i, :nv].view(np.uint64), out["vad_energy"][i, :nv].view(np.uint64)), what
            assert np.array_equal(base["vad_zcr"][i, :nv], out["vad_zcr"][i, :nv]), what
    assert tally["cells"] == 15 * len(clips) * len(fc.LEADS)  # every clip of every launch was checked
