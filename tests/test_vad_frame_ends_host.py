"""The pass-A corpus (tests/vad_frame_end_cases.py) is what tests/test_gpu_vad_frame_ends.py needs it
to be, checked on the CPU: over its (L, S, n, lead) set the frame starts and the frame ends each
land on every element of a word, on the aligned element and in both halves; the -32768 runs lie in
the kept part, in the dropped part and across the boundary of the half-words the kernel reads, for
runs of one, two and four samples; the short-frame groups hold frames inside one word and over two;
and the C oracle gives every clip status 0, so the GPU test may skip none."""
import numpy as np
import pytest

import edge_corpus as ec
import oracle
import vad_frame_end_cases as fc


@pytest.fixture(scope="module")
def clips():
    return fc.corpus()


def _boundaries(c, lead):
    L, S = fc.GROUPS[c.group]
    for f in range(fc.n_vad_frames(c.pcm.size, L, S)):
        for end in (0, 1):
            yield f, end, fc.boundary(lead, L, S, f, end)


def test_shapes(clips):
    assert {c.group for c in clips} == set(fc.GROUPS)
    for g in ("p1102", "p1024"):
        L, S = fc.GROUPS[g]
        sizes = {c.pcm.size for c in clips if c.group == g}
        assert sizes == {L + 31 * S, L + 31 * S + 17, L}, g
        for n in sizes:  # n = L + 31 S: the last frame ends on the clip's last sample; + 17: samples left over
            nv = fc.n_vad_frames(n, L, S)
            assert nv == (1 if n == L else 32) and n - ((nv - 1) * S + L) in (0, 17)
    for c in clips:
        L, S = fc.GROUPS[c.group]
        assert 1 <= fc.n_vad_frames(c.pcm.size, L, S) <= 128, c  # the FAST layout's frame capacity
        assert ec.fast_layout(c.pcm.size, L, S) == 1, c
        assert (c.pcm == fc.NEG).sum() == sum(r for _, r in c.runs), c
        for a, r in c.runs:
            assert (c.pcm[a:a + r] == fc.NEG).all(), c


def test_every_element_both_halves(clips):
    """Starts on every element 0 .. 31 (0: aligned), ends on every element 1 .. 32 (32: aligned)."""
    hit = {0: set(), 1: set()}
    per_group = {}
    for c in clips:
        for lead in fc.LEADS:
            for f, end, (w, e, kept, dropped) in _boundaries(c, lead):
                hit[end].add(e)
                per_group.setdefault((c.group, end), set()).add(e)
                assert (kept is None) == (e == 32 * end)
                if kept is not None:  # the kept and dropped elements make up one 16-sample half
                    lo, hi = min(kept[0], dropped[0]), max(kept[1], dropped[1])
                    assert (lo, hi) == ((0, 16) if e <= 16 else (16, 32))
                    assert kept[1] - kept[0] + dropped[1] - dropped[0] == 16 and kept[1] > kept[0]
    assert hit[0] == set(range(32)) and hit[1] == set(range(1, 33))
    # 441 = 25 mod 32 is coprime to 32: the production group alone covers everything; with S = 512
    # only the lead moves a boundary
    assert per_group[("p1102", 0)] == set(range(32)) and per_group[("p1102", 1)] == set(range(1, 33))
    assert per_group[("p1024", 0)] == set(range(8)) and per_group[("p1024", 1)] == set(range(1, 8)) | {32}


def test_first_and_last_word(clips):
    """Frame 0 starts inside the clip's first word at leads 1 .. 7, and a last frame that ends on the
    clip's last sample ends inside its last word."""
    for g in ("p1102", "p1024"):
        L, S = fc.GROUPS[g]
        n = L + 31 * S
        starts = {fc.boundary(lead, L, S, 0, 0)[:2] for lead in fc.LEADS}
        assert starts == {(0, lead) for lead in fc.LEADS}
        for lead in fc.LEADS:
            w, e, kept, _ = fc.boundary(lead, L, S, 31, 1)
            assert w == (lead + n - 1) // 32 and 32 * w + e == lead + n
        assert any(fc.boundary(lead, L, S, 31, 1)[2] is not None for lead in fc.LEADS)


def test_negative_runs_cover_the_half_words(clips):
    """Runs of 1 / 2 / 4 samples in the kept part, in the dropped part and across the boundary (2 / 4),
    for starts and for ends; a kept run of four on an aligned group (u = 0 mod 4: the 32-bit square
    chain wraps) at some lead."""
    seen, wrapped = set(), False
    for c in clips:
        L, S = fc.GROUPS[c.group]
        for lead in fc.LEADS:
            for f, end, _ in _boundaries(c, lead):
                for a, r in c.runs:
                    place = fc.run_place(lead, L, S, f, end, a, r)
                    if place:
                        seen.add((r, end, place))
                        wrapped |= r == 4 and place == "kept" and (lead + a) % 4 == 0
    want = {(r, end, p) for r in fc.RUNS for end in (0, 1) for p in ("kept", "dropped", "straddle")
            if not (r == 1 and p == "straddle")}
    assert want <= seen, want - seen
    assert wrapped


def test_short_frames(clips):
    """L = 20 and L = 2: frames that start and end in one word, and frames over two adjacent words."""
    for g in ("l20", "l2"):
        L, S = fc.GROUPS[g]
        assert L < 32
        span = set()
        for c in fc.group_clips(g):
            for lead in fc.LEADS:
                for f in range(fc.n_vad_frames(c.pcm.size, L, S)):
                    span.add(fc.boundary(lead, L, S, f, 1)[0] - fc.boundary(lead, L, S, f, 0)[0])
        assert span == {0, 1}, (g, span)


def test_oracle_status(clips):
    from src.pipeline import create_window
    for c in clips:
        L, S = fc.GROUPS[c.group]
        r = oracle.process_clip(c.pcm, L, S, create_window(fc.WINDOW, L), do_vad=True)
        assert r["status"] == 0 == c.status, c
        assert len(r["vad_energy"]) == fc.n_vad_frames(c.pcm.size, L, S), c
        assert np.isfinite(r["feat"]).all(), c
