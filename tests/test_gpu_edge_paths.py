"""The edge-clip corpus (tests/edge_corpus.py) through all three extraction paths, each against the
C oracle: FAST (extract_kernel<true>, leads 0-7), the generic layout (extract_kernel<false>: the
same clips under an explicit max_len past the FAST capacity, leads 0 and 5) and the general kernel
(dsp_extract_general, leads 0 and 5).  dsp_extract_fast_layout says which fused layout a launch
takes, so no launch can drift to the other one unnoticed.

Per launch and clip, against the oracle (the project's tolerances): status,
start/end, n_frames, every per-frame ZCR and VAD ZCR exact; VAD energies 1e-12 relative; per-frame
E / M 1e-5 relative; the 15-d vector through feat_close.  Across leads within a path, and across
the paths, feat / seq / start_end / n_frames / status are bit-identical.  A clip is left out of the
value checks only when the corpus declares a nonzero status for it (pinned on the CPU by
test_edge_corpus_host.py), and the absolute term of feat_close may carry near-zero statistics only.
"""
import numpy as np
import pytest

import edge_corpus as ec
import oracle
from test_gpu_extract import feat_close

pytestmark = pytest.mark.gpu

LEADS = {"fast": tuple(range(8)), "generic": (0, 5), "general": (0, 5)}
CASES = [(g, vad) for g in ec.GROUPS for vad in (True, False)]
_REFS, _RUNS = {}, {}


def _refs(group, vad):
    """Oracle results of the group's clips, computed once and shared by every launch."""
    key = (group, vad)
    if key not in _REFS:
        from src.pipeline import create_window
        L, S = ec.GROUPS[group]
        w = create_window(ec.WINDOW, L)
        _REFS[key] = {c.name: oracle.process_clip(c.pcm, L, S, w, do_vad=vad) for c in ec.corpus() if c.group == group}
    return _REFS[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_launch(out, clips, refs, vad, tag, tally):
    """One launch against the oracle, clip by clip."""
    for i, c in enumerate(clips):
        r = refs[c.name]
        what = tag + (c.name,)
        assert r["status"] == c.status, what
        assert (out["status"][i] & 0xFF) == c.status, (what, out["status"][i])
        if c.status:
            continue
        assert tuple(out["start_end"][i]) == (r["start"], r["end"]), (what, out["start_end"][i], r["start"], r["end"])
        F = r["n_frames"]
        assert out["n_frames"][i] == F, (what, out["n_frames"][i], F)
        seq = out["seq"][i, :F]
        np.testing.assert_array_equal(seq[:, 2], r["seq"][:, 2], err_msg=str(what))
        np.testing.assert_allclose(seq[:, 0], r["seq"][:, 0], rtol=1e-5, atol=1e-30, err_msg=str(what))
        np.testing.assert_allclose(seq[:, 1], r["seq"][:, 1], rtol=1e-5, atol=1e-30, err_msg=str(what))
        if vad:
            nv = len(r["vad_energy"])
            np.testing.assert_array_equal(out["vad_zcr"][i, :nv], r["vad_zcr"], err_msg=str(what))
            np.testing.assert_allclose(out["vad_energy"][i, :nv], r["vad_energy"], rtol=1e-12, atol=0, err_msg=str(what))
        got, ref = np.asarray(out["feat"][i], np.float64), r["feat"]
        assert np.isfinite(got).all() and np.isfinite(ref).all(), (what, got, ref)
        assert not feat_close(got, ref).any(), (what, got, ref)
        # cells that pass only through feat_close's absolute term: near-zero statistics only
        scale = np.repeat(np.abs(ref[[0, 5, 10]]), 5)
        rel_bad = np.abs(got - ref) > 1e-5 * np.abs(ref) + 1e-30
        assert (np.abs(ref[rel_bad]) < 1e-3 * scale[rel_bad]).all(), (what, np.nonzero(rel_bad)[0], got, ref)
        tally["abs_cells"] += int(rel_bad.sum())
        tally["cells"] += ref.size


def _same_bits(a, ia, b, ib, F, what):
    """Clip ia of launch a and clip ib of launch b: identical results to the bit."""
    assert np.array_equal(_bits(a["feat"][ia]), _bits(b["feat"][ib])), (what, "feat", a["feat"][ia], b["feat"][ib])
    assert np.array_equal(a["start_end"][ia], b["start_end"][ib]), (what, "start_end")
    assert a["n_frames"][ia] == b["n_frames"][ib], (what, "n_frames")
    assert (a["status"][ia] & 0xFF) == (b["status"][ib] & 0xFF), (what, "status")
    assert np.array_equal(_bits(a["seq"][ia, :F]), _bits(b["seq"][ib, :F])), (what, "seq")


def _run_group(group, vad):
    """Every launch of one group: FAST at leads 0-7, generic layout and general kernel at leads 0 and
    5; each launch against the oracle, then bitwise across leads and across paths."""
    key = (group, vad)
    if key in _RUNS:
        return _RUNS[key]
    import torch
    from src.pipeline import FeatureExtractor
    from test_gpu_general import _general
    L, S = ec.GROUPS[group]
    refs = _refs(group, vad)
    tally = dict(abs_cells=0, cells=0, redo=0, clips=0, launches=0)
    fx = FeatureExtractor(L, S, ec.WINDOW, vad, return_vad_lists=True, return_sequences=True)
    cap = fx.fused_cap()
    assert cap == ec.fused_cap(L, S)
    base = {}
    for path in ec.PATHS:
        clips = ec.group_clips(group, path)
        if not clips:
            continue
        longest = max(c.pcm.size for c in clips)
        for lead in LEADS[path]:
            pcm, off = ec.pack(clips, lead)
            if path == "fast":
                assert ec.fast_layout(longest, L, S) == 1, (group, longest)
                out = fx(torch.as_tensor(pcm).cuda(), off)
            elif path == "generic":
                # the same kind of launch under a max_len the compile-time layout cannot hold
                max_len = max(longest, ec.fast_cap(L, S) + 1)
                assert max_len <= cap and ec.fast_layout(max_len, L, S) == 0 and ec.lds_bytes(max_len, L, S) > 0
                out = fx(torch.as_tensor(pcm).cuda(), off, max_len=max_len)
            if path == "general":
                out = _general(pcm, off, L, S, ec.WINDOW, vad)
            else:
                out = {k: v.cpu().numpy().copy() for k, v in out.items()}
            tag = (group, "vad" if vad else "novad", path, lead)
            _check_launch(out, clips, refs, vad, tag, tally)
            tally["launches"] += 1
            if path not in base:
                base[path] = (clips, out)
                continue
            for i, c in enumerate(clips):
                if not c.status:
                    _same_bits(base[path][1], i, out, i, refs[c.name]["n_frames"], tag + (c.name, "vs lead 0"))
    # across the paths: a clip's results do not depend on the kernel that computed them
    paths = list(base)
    for a in range(len(paths)):
        for b in range(a + 1, len(paths)):
            ca, oa = base[paths[a]]
            cb, ob = base[paths[b]]
            ib = {c.name: i for i, c in enumerate(cb)}
            for i, c in enumerate(ca):
                if c.name in ib and not c.status:
                    _same_bits(oa, i, ob, ib[c.name], refs[c.name]["n_frames"], (group, vad, paths[a], paths[b], c.name))
    # how much of the group the exact (numpy-order) redo kernel saw: each clip on the first path it takes
    seen = set()
    for path in paths:
        clips, out = base[path]
        for i, c in enumerate(clips):
            if c.name not in seen:
                seen.add(c.name)
                tally["clips"] += 1
                tally["redo"] += int(bool(out["status"][i] & 0x100))
    assert seen == {c.name for c in ec.corpus() if c.group == group}  # no clip without a launch
    _RUNS[key] = tally
    return tally


@pytest.mark.parametrize("group,vad", CASES, ids=["%s-%s" % (g, "vad" if v else "novad") for g, v in CASES])
def test_corpus_paths_vs_oracle(group, vad):
    t = _run_group(group, vad)
    print("%s vad=%d: %d launches, %d clips, %d redone exactly, %d of %d cells on the absolute term"
          % (group, vad, t["launches"], t["clips"], t["redo"], t["abs_cells"], t["cells"]))
    assert t["clips"] > 0 and t["launches"] >= 4


def test_corpus_counts():
    """The two figures DESIGN.md §2 records: the 15-d cells that passed only through feat_close's
    absolute term (each asserted near zero in _check_launch: |ref| < 1e-3 x its group's mean) and
    the corpus clips that came back with the redo bit (status & 0x100)."""
    tot = dict(abs_cells=0, cells=0, redo=0, clips=0, launches=0)
    for group, vad in CASES:
        for k, v in _run_group(group, vad).items():
            tot[k] += v
    print("edge corpus: cells needing the absolute term: %d of %d (%d launches)"
          % (tot["abs_cells"], tot["cells"], tot["launches"]))
    print("edge corpus: clips redone on the exact path (status & 0x100): %d of %d (clip, endpoint detection on/off)"
          % (tot["redo"], tot["clips"]))
    assert tot["clips"] == 2 * len(ec.corpus())
