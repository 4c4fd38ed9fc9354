"""The edge-clip corpus (tests/edge_corpus.py) is what it claims to be, checked on the CPU: every
clip gets its declared status and frame counts from the C oracle, the -32768 clips hold an aligned
group of four at exactly the leads they claim, and the boundary clips sit on their boundary.  A
later edit of the corpus that empties a case fails here, not silently on the GPU."""
import numpy as np
import pytest

import edge_corpus as ec
import oracle


@pytest.fixture(scope="module")
def clips():
    return ec.corpus()


def test_corpus_shape(clips):
    assert 40 <= len(clips) < 100
    assert {c.group for c in clips} == set(ec.GROUPS)
    for c in clips:
        assert c.pcm.dtype == np.int16 and c.pcm.ndim == 1 and c.pcm.size > 0, c
        assert c.purpose and set(c.paths) <= set(ec.PATHS) and c.paths, c
    L, S = ec.GROUPS["main"]
    assert max(c.pcm.size for c in clips) == ec.fused_cap(L, S) + 1
    # deterministic: a second build gives the same samples
    ec._CORPUS, first = None, clips
    try:
        again = ec.corpus()
        assert [(c.group, c.name) for c in again] == [(c.group, c.name) for c in first]
        assert all(np.array_equal(a.pcm, b.pcm) for a, b in zip(again, first))
    finally:
        ec._CORPUS = first


def test_oracle_status_and_frame_counts(clips):
    from src.pipeline import create_window
    pinned_nv = pinned_F = 0
    for c in clips:
        L, S = ec.GROUPS[c.group]
        w = create_window(ec.WINDOW, L)
        on = oracle.process_clip(c.pcm, L, S, w, do_vad=True)
        off = oracle.process_clip(c.pcm, L, S, w, do_vad=False)
        assert on["status"] == c.status and off["status"] == c.status, c
        assert np.isfinite(on["feat"]).all() and np.isfinite(off["feat"]).all(), c
        if c.nv is not None:
            assert len(on["vad_energy"]) == c.nv, (c, len(on["vad_energy"]))
            pinned_nv += 1
        if c.F is not None:
            assert off["n_frames"] == c.F == len(off["seq"]), (c, off["n_frames"])
            pinned_F += 1
    assert pinned_nv >= 30 and pinned_F >= 30


def test_frame_count_cases_present(clips):
    """Both sides of every threshold of the FAST kernel's frame-count paths (1 / 32 / 64 / 128)."""
    fr = [c for c in clips if c.group == "frames"]
    assert {1, 2, 9, 10, 11, 63, 64, 65, 127, 128, 129} <= {c.nv for c in fr}
    L, S = ec.GROUPS["frames"]
    for F in (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129):
        exact = [c for c in fr if c.F == F and c.pcm.size == L + (F - 1) * S]
        padded = [c for c in fr if c.F == F and c.pcm.size != L + (F - 1) * S]
        assert exact and padded, F
        for c in padded:  # the last frame starts inside the clip and runs past its end
            last = (F - 1) * S
            assert last < c.pcm.size < last + L or F == 1 and c.pcm.size < L, c
    for c in fr:  # 129 frames of either kind never fit the FAST layout, 128 do
        big = (c.nv or 0) > 128 or (c.F or 0) > 128
        assert ("fast" in c.paths) == (not big), c
        assert ec.fast_layout(c.pcm.size, L, S) == (0 if big else 1), c
    # the tied variants: every full frame of the tone is the same samples; +-1 changes a few
    for nv in (64, 65, 128):
        tied = next(c for c in fr if c.name == "nv%d_tied" % nv)
        pm1 = next(c for c in fr if c.name == "nv%d_tied_pm1" % nv)
        assert np.array_equal(tied.pcm[:L], tied.pcm[S:S + L]) and np.array_equal(tied.pcm[:-S], tied.pcm[S:])
        d = pm1.pcm.astype(np.int64) - tied.pcm
        assert np.abs(d).max() == 1 and 10 <= np.count_nonzero(d) < nv


def test_negative_full_scale_groups(clips):
    """Buffer coordinates u = lead + j: the FAST kernel's 32-bit square chain covers the four samples
    at u = 0 mod 4 and wraps when all four are -32768."""
    claimed = [c for c in clips if c.wrap_leads is not None]
    assert len(claimed) >= 10
    for c in claimed:
        assert (c.pcm == ec.NEG).any(), c  # kneg is set
        assert ec.aligned_wrap_leads(c.pcm) == tuple(c.wrap_leads), (c, ec.aligned_wrap_leads(c.pcm))
        for lead in c.wrap_leads:  # spelled out once more, without the helper
            u = np.arange(c.pcm.size) + lead
            g0 = np.nonzero((u % 4 == 0) & (u + 3 < lead + c.pcm.size))[0]
            assert any((c.pcm[j:j + 4] == ec.NEG).all() for j in g0), (c, lead)
    for c in clips:
        if c.wrap_leads is None:
            assert not (c.pcm == ec.NEG).any(), c  # an unclaimed clip holds no -32768 at all
    by = {c.name: c for c in clips if c.group == "main"}
    assert by["neg_single"].wrap_leads == () and np.count_nonzero(by["neg_single"].pcm == ec.NEG) == 1
    r4 = by["neg_run4_aligned"]
    j = np.nonzero(r4.pcm == ec.NEG)[0]
    assert j.size == 4 and j[0] % 4 == 0 and (np.diff(j) == 1).all() and tuple(r4.wrap_leads) == (0, 4)
    # the frame-edge runs leave a wrapped group inside a partial word of a VAD frame end at most leads
    L, S = ec.GROUPS["main"]
    e = by["neg_runs_frame_edges"].pcm
    for f in (0, 2, 4):
        assert (e[f * S + L - 6:f * S + L + 6] == ec.NEG).all() and (e[max(f * S - 6, 0):f * S + 6] == ec.NEG).all()
    assert (by["neg_all"].pcm == ec.NEG).all()
    assert np.count_nonzero(by["neg_all_one_max"].pcm != ec.NEG) == 1 and by["neg_all_one_max"].pcm.max() == 32767


def test_boundary_clips_sit_on_the_boundary(clips):
    seen = set()
    for c in clips:
        if c.boundary is None:
            continue
        L, S = ec.GROUPS[c.group]
        kind, side = c.boundary
        n = c.pcm.size
        seen.add((c.group, kind, side))
        if kind == "fast" and side == 0:
            assert ec.fast_layout(n, L, S) == 1 and ec.fast_layout(n + 1, L, S) == 0, c
            assert "fast" in c.paths
        elif kind == "fast":
            assert ec.fast_layout(n, L, S) == 0 and ec.fast_layout(n - 1, L, S) == 1, c
            assert ec.lds_bytes(n, L, S) > 0 and "fast" not in c.paths and "generic" in c.paths
        elif side == 0:
            assert ec.lds_bytes(n, L, S) > 0 and ec.lds_bytes(n + 1, L, S) == 0, c
            assert "generic" in c.paths
        else:
            assert ec.lds_bytes(n, L, S) == 0 and ec.lds_bytes(n - 1, L, S) > 0, c
            assert c.paths == ("general",)
    assert seen == {("main", "fast", 0), ("main", "fast", 1), ("main", "fused", 0), ("main", "fused", 1),
                    ("frames", "fast", 0), ("frames", "fast", 1)}
    assert ec.FAST_MAX_LEN == ec.fast_cap(*ec.GROUPS["main"]) == 49145
    # the frame-length groups: 1260 is the longest FAST frame, 1261 never launches FAST
    assert ec.fast_cap(*ec.GROUPS["lcap"]) == ec.FAST_MAX_LEN and ec.fast_cap(*ec.GROUPS["lcap1"]) == 0
    assert ec.GROUPS["lcap1"][0] == ec.GROUPS["lcap"][0] + 1
    assert all("fast" not in c.paths for c in clips if c.group == "lcap1")
    assert ec.GROUPS["lshift"][0] == ec.GROUPS["lshift"][1]


def test_zcr_and_sum_clips(clips):
    by = {c.name: c for c in clips if c.group == "main"}
    a = by["zcr_alternating"].pcm.astype(np.int64)
    assert a.size >= 8192 and (a[-2048:-1] * a[-2047:] < 0).all()  # alternating to the last sample
    for per in (4096, 64):
        x = by["zcr_square_%d" % per].pcm.astype(np.int64)
        ch = np.nonzero(x[:-1] * x[1:] < 0)[0] + 1  # first sample after each change
        assert ch.size >= 3 and (ch % (per // 2) == 0).all()
    h = by["zcr_half_at_mean"].pcm.astype(np.int64)
    assert h.sum() == 0 and np.count_nonzero(h == 0) * 2 == h.size
    m = by["zcr_mean_half_integer"].pcm.astype(np.int64)
    assert 2 * m.sum() == 15 * m.size and (m == 7).any() and (m == 8).any()
    d = by["dc_heavy"].pcm.astype(np.int64)
    assert 31980 < d.mean() < 32000 and np.abs(d[:5000] - 31990).max() <= 3 and np.abs(d - 31990).max() > 300
    for name, sign in (("sum_max_pos", 1), ("sum_max_neg", -1)):
        x = by[name].pcm.astype(np.int64)
        assert x.size == ec.FAST_MAX_LEN and 0.59 * 2 ** 31 < sign * x.sum() < 2 ** 31
