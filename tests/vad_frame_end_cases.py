"""Clips aimed at the FAST extraction kernel's pass A, the exact moments of the VAD frames (a plain
helper module, no fixtures; tests/test_vad_frame_ends_host.py pins it on the CPU,
tests/test_gpu_vad_frame_ends.py runs it).

Buffer coordinates as in edge_corpus: a clip packed at lead = offset mod 8 has its sample j at
buffer sample u = lead + j, in 32-sample words.  VAD frame f covers u0 = lead + f S .. u1 = u0 + L.
The kernel sums whole-word totals over the frame's words and takes off what the first and the last
word hold outside the frame.  For that it reads, per frame end, the 16-sample half-word holding the
boundary and sums its `kept` elements (`boundary` below): a start sits at element e = u0 mod 32 of
word u0 div 32 (e = 0: aligned, nothing read); an end at e = u1 - 32 w = 1 .. 32 of the frame's last
word w = (u1 - 1) div 32 (e = 32: aligned).  For e <= 16 the kept elements are [0, e) of the word,
otherwise [e, 32); the half-word's other elements are `dropped`.
"""
import numpy as np

from edge_corpus import NEG

WINDOW = "hamming"
GROUPS = {                # launch groups: (frame_length, frame_shift)
    "p1102": (1102, 441),  # the production frame: 441 = 25 mod 32 is coprime to 32, so 32 frames at any
                           # one lead put a start and an end on every element of a word
    "p1024": (1024, 512),  # every boundary of a clip on the same element: the lead alone moves it
    "l20": (20, 7),        # frames inside one word, and over two (wa + 1 == wb)
    "l2": (2, 1),          # the shortest frame that can span two words (the FAST layout takes it)
}
LEADS = tuple(range(8))
RUNS = (1, 2, 4)          # adjacent -32768 samples
PLACES = ("before", "after", "straddle")  # of a frame boundary b: [b - r, b), [b, b + r), [b - r // 2, ..)


class Clip:
    def __init__(self, name, group, pcm, runs=()):
        pcm = np.asarray(pcm)
        assert pcm.min() >= -32768 and pcm.max() <= 32767, name
        self.name, self.group = name, group
        self.pcm = np.ascontiguousarray(pcm.astype(np.int16))
        self.pcm.setflags(write=False)
        self.runs = tuple(runs)  # (first sample, length) of each -32768 run
        self.status = 0          # every clip is an ordinary one for the oracle (pinned by the host test)

    def __repr__(self):
        return "Clip(%s/%s, n=%d)" % (self.group, self.name, self.pcm.size)


def n_vad_frames(n, L, S):
    return (n - L) // S + 1 if n >= L else 0


def boundary(lead, L, S, f, end):
    """Frame f's start (end = 0) or end (1) in buffer coordinates -> (word w, element e, kept, dropped):
    the element ranges (first, last + 1) of word w that pass A sums / leaves out of the half-word it
    reads (both None for an aligned boundary, which reads nothing)."""
    u0 = lead + f * S
    if end:
        u1 = u0 + L
        w = (u1 - 1) // 32
        e = u1 - 32 * w
    else:
        w, e = u0 // 32, u0 % 32
    if e == (32 if end else 0):
        return w, e, None, None
    if e <= 16:
        return w, e, (0, e), (e, 16)
    return w, e, (e, 32), (16, e)


def run_place(lead, L, S, f, end, first, length):
    """Where the -32768 run [first, first + length) of a clip lies in the half-word of one boundary:
    'kept', 'dropped', 'straddle' (samples on both sides), or None (not wholly inside the half-word)."""
    w, e, kept, dropped = boundary(lead, L, S, f, end)
    if kept is None:
        return None
    a, b = lead + first - 32 * w, lead + first + length - 32 * w  # the run in the word's elements
    half = (0, 16) if e <= 16 else (16, 32)
    if a < half[0] or b > half[1]:
        return None
    if kept[0] <= a and b <= kept[1]:
        return "kept"
    if dropped[0] <= a and b <= dropped[1]:
        return "dropped"
    return "straddle"


def _speech(seed, n):
    from src.synth import make_clip
    x = make_clip(seed, max(n, 2048)).astype(np.int64)[:n]
    assert x.min() > NEG
    return x


def _with_runs(x, L, S, r, step=1):
    """Runs of r samples at -32768 around the boundaries of every step-th frame of clip x, the place
    cycling from one boundary to the next: before the boundary, after it, across it (r >= 2)."""
    x = x.copy()
    n, runs = x.size, []
    places = PLACES if r > 1 else PLACES[:2]
    k = 0
    for f in range(0, n_vad_frames(n, L, S), step):
        for b in (f * S, f * S + L):
            place = places[k % len(places)]
            k += 1
            a = b - r if place == "before" else b if place == "after" else b - r // 2
            a = min(max(a, 0), n - r)
            if any(a < p + q + 1 and p < a + r + 1 for p, q in runs):  # keep the runs apart
                continue
            x[a:a + r] = NEG
            runs.append((a, r))
    return x, runs


_CORPUS = None


def corpus():
    """The clips of every group, built once per process."""
    global _CORPUS
    if _CORPUS is None:
        clips = []
        seed = 9900
        for g in ("p1102", "p1024"):
            L, S = GROUPS[g]
            for tag, n in (("f32", L + 31 * S), ("f32_tail17", L + 31 * S + 17), ("f1", L)):
                seed += 1
                base = _speech(seed, n)
                clips.append(Clip(tag, g, base))
                for r in RUNS:
                    x, runs = _with_runs(base, L, S, r)
                    clips.append(Clip("%s_neg%d" % (tag, r), g, x, runs))
        for g, nv in (("l20", 120), ("l2", 120)):
            L, S = GROUPS[g]
            seed += 1
            n = L + (nv - 1) * S
            base = _speech(seed, n)
            clips.append(Clip("nv%d" % nv, g, base))
            clips.append(Clip("nv%d_tail" % nv, g, _speech(seed + 50, n + S - 1)))  # S - 1 samples left over
            for r in RUNS:
                x, runs = _with_runs(base, L, S, r, step=5)
                clips.append(Clip("nv%d_neg%d" % (nv, r), g, x, runs))
        names = [(c.group, c.name) for c in clips]
        assert len(set(names)) == len(names)
        _CORPUS = clips
    return _CORPUS


def group_clips(group):
    return [c for c in corpus() if c.group == group]
