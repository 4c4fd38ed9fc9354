"""The edge-clip corpus: named, deterministic int16 clips aimed at the code of the three extraction
paths that ordinary speech-like clips never reach (a plain helper module, no fixtures).

  FAST     extract_kernel<true>: compile-time LDS layout, the clip in registers
  generic  extract_kernel<false>: the same fused kernel on the runtime carve
  general  dsp_extract_general: one workgroup per clip from global memory

Each clip belongs to one launch group (a frame length / shift), says what it is for, which paths
can take it, the oracle status it must get, and -- where the clip exists to hit a frame count -- its
number of VAD frames `nv` (endpoint detection on) and of feature frames `F` (endpoint detection
off).  tests/test_edge_corpus_host.py pins those declarations against the C oracle on the CPU;
tests/test_gpu_edge_paths.py runs every group through every path.

Buffer coordinates: the kernels address a clip in 8-sample vectors of the packed buffer, so a clip
that starts at offset o sits at lead = o mod 8 and its sample j is buffer sample u = lead + j.  The
FAST kernel squares samples in groups of four at u = 0 mod 4 (one 32-bit chain per group), which
wraps to 0 exactly when all four are -32768: `wrap_leads` lists the leads at which a clip holds such
a group.
"""
import numpy as np

WINDOW = "hamming"
GROUPS = {            # launch groups: (frame_length, frame_shift)
    "main": (1102, 441),    # the production frame; clips up to the capacities of both fused layouts
    "frames": (882, 220),   # frame counts on either side of 1 / 32 / 64 / 128 (FAST holds 128)
    "lcap": (1260, 441),    # the longest frame the FAST window table holds
    "lcap1": (1261, 441),   # one past it: every launch runs the generic layout
    "lshift": (441, 441),   # frame_length == frame_shift
}
FAST_WORDS = 1536  # EXTRACT_THREADS x EXTRACT_RREG 32-sample words, the 7-sample lead included
FAST_MAX_LEN = FAST_WORDS * 32 - 7  # 49145: the longest FAST clip wherever the frame caps allow it
PATHS = ("fast", "generic", "general")
NEG = -32768


class EdgeClip:
    def __init__(self, name, group, pcm, purpose, paths=PATHS, status=0, nv=None, F=None, wrap_leads=None,
                 boundary=None):
        pcm = np.asarray(pcm)
        assert pcm.min() >= -32768 and pcm.max() <= 32767, name
        self.name, self.group, self.purpose = name, group, purpose
        self.pcm = np.ascontiguousarray(pcm.astype(np.int16))
        self.paths = tuple(paths)
        self.status = status          # oracle status, endpoint detection on and off alike
        self.nv = nv                  # VAD frames with endpoint detection on (None: not pinned)
        self.F = F                    # feature frames with endpoint detection off (None: not pinned)
        self.wrap_leads = wrap_leads  # leads 0..7 with an aligned group of four -32768 (None: no claim)
        self.boundary = boundary      # ("fast" | "fused", 0: the last length inside, 1: the first outside)

    def __repr__(self):
        return "EdgeClip(%s/%s, n=%d)" % (self.group, self.name, self.pcm.size)


def lds_bytes(n, L, S):
    from src import _hip
    return _hip.lib().dsp_extract_lds_bytes(int(n), L, S)


def fast_layout(n, L, S):
    from src import _hip
    return _hip.lib().dsp_extract_fast_layout(int(n), L, S)


def _last_true(pred, lo, hi):
    """Largest n in [lo, hi] with pred(n), for a predicate that is true up to some n and false after."""
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


def fused_cap(L, S):
    """Longest clip the fused kernel holds (FeatureExtractor.fused_cap without a device)."""
    return _last_true(lambda n: lds_bytes(n, L, S) > 0, 0, 1 << 24)


def fast_cap(L, S):
    """Longest max_len that still launches the FAST layout (0: none)."""
    return _last_true(lambda n: n == 0 or fast_layout(n, L, S) == 1, 0, 1 << 24)


def aligned_wrap_leads(pcm):
    """Leads 0..7 at which four consecutive -32768 samples share a group at u = lead + j = 0 mod 4."""
    neg = (np.asarray(pcm) == NEG).astype(np.int64)
    if neg.size < 4:
        return ()
    run4 = neg[:-3] + neg[1:-2] + neg[2:-1] + neg[3:] == 4  # run4[j]: samples j .. j + 3
    j = np.nonzero(run4)[0]
    return tuple(lead for lead in range(8) if ((j + lead) % 4 == 0).any())


def _speech(seed, n):
    from src.synth import make_clip
    return make_clip(seed, n).astype(np.int64)


def _quiet(seed, n):
    return np.random.default_rng(seed).integers(-20, 21, n)


def _tone(n, period, amp, phase=0.0):
    return np.round(amp * np.sin(2 * np.pi * (np.arange(n) + phase) / period)).astype(np.int64)


def _main_clips():
    L, S = GROUPS["main"]
    g = "main"
    out = []
    n = 16000
    nv = (n - L) // S + 1
    base = _speech(9100, n)
    assert base.min() > NEG

    # ---- full-scale negative runs (kneg) ----
    x = base.copy()
    for f in range(0, nv, 2):
        for edge in (f * S, f * S + L):
            x[max(edge - 6, 0):min(edge + 6, n)] = NEG
    out.append(EdgeClip("neg_runs_frame_edges", g, x, "12-sample -32768 runs across every second VAD frame "
                        "start and end: wrapped groups in interior words and in pass A's partial words",
                        wrap_leads=tuple(range(8))))
    x = base.copy()
    x[5003] = NEG
    out.append(EdgeClip("neg_single", g, x, "one -32768 sample: kneg set, nothing wraps", wrap_leads=()))
    x = np.where((np.arange(n) // 50) % 2 == 0, 32767, NEG)
    x[:3000] = _quiet(1, 3000)
    out.append(EdgeClip("neg_square_fullscale", g, x, "+32767 / -32768 square wave, half period 50, quiet lead-in",
                        wrap_leads=tuple(range(8))))
    out.append(EdgeClip("neg_all", g, np.full(n, NEG), "all -32768: every group wraps, constant signal",
                        wrap_leads=tuple(range(8))))
    x = np.full(n, NEG)
    x[7001] = 32767
    out.append(EdgeClip("neg_all_one_max", g, x, "all -32768 with one +32767", wrap_leads=tuple(range(8))))
    x = np.full(n, NEG)
    x[6000:10000] += 6000 + _tone(4000, 100, 6000)
    out.append(EdgeClip("neg_floor_burst", g, x, "-32768 floor with a tone burst: strongly negative mean",
                        wrap_leads=tuple(range(8))))
    x = base.copy()
    x[4000:4004] = NEG
    out.append(EdgeClip("neg_run4_aligned", g, x, "a run of exactly four at a clip position that is a multiple "
                        "of 4: one aligned group at leads 0 and 4 only", wrap_leads=(0, 4)))
    x = base.copy()
    x[4096:4160] = NEG
    out.append(EdgeClip("neg_run64", g, x, "a run of 64 covering whole words", wrap_leads=tuple(range(8))))

    # ---- 32-bit clip sum at the FAST capacity ----
    for name, fill in (("sum_max_pos", 32767), ("sum_max_neg", NEG)):
        x = np.full(FAST_MAX_LEN, fill)
        x[20000:30000] = _tone(10000, 100, 20000)
        out.append(EdgeClip(name, g, x, "the longest FAST clip at full scale: |K| = 39145 x 32768, 0.6 x 2^31",
                            wrap_leads=tuple(range(8)) if fill == NEG else None, boundary=("fast", 0)))

    # ---- ZCR structure ----
    n = 12000
    x = np.where(np.arange(n) % 2 == 0, 9000, -9000)
    x[:1000] = _quiet(2, 1000)
    out.append(EdgeClip("zcr_alternating", g, x, "a sign change at every sample up to the clip's end: the densest "
                        "input of the u16 segment prefixes"))
    n = 16000
    for per in (4096, 64):
        x = np.where((np.arange(n) // (per // 2)) % 2 == 0, 10000, -10000)
        out.append(EdgeClip("zcr_square_%d" % per, g, x, "sign changes at multiples of %d: on word%s boundaries at "
                            "lead 0" % (per // 2, " and 64-word segment" if per == 4096 else "")))
    x = np.tile(np.array([7000, 0, -7000, 0]), 2000)
    out.append(EdgeClip("zcr_half_at_mean", g, x, "(+A, 0, -A, 0): the mean is exactly 0 and half the samples equal it"))
    x = np.tile(np.array([3001, -3000, 1, 0, 1, 0, 0, 1]) + 7, 1000)
    out.append(EdgeClip("zcr_mean_half_integer", g, x, "mean exactly 7.5 with samples at 7 and 8 (tpos / t0)"))

    # ---- DC-heavy, tiny AC ----
    n = 12000
    x = 31990 + np.random.default_rng(3).integers(-3, 4, n)
    x[5000:8000] += _tone(3000, 60, 400)
    out.append(EdgeClip("dc_heavy", g, x, "mean ~31990, AC +-3 with a +-400 burst: double-double VAD energy, fp32 "
                        "centring"))

    # ---- capacity boundaries ----
    cap = fused_cap(L, S)
    out.append(EdgeClip("len_fast_cap", g, _speech(9201, FAST_MAX_LEN), "the longest FAST launch", boundary=("fast", 0)))
    out.append(EdgeClip("len_fast_cap_plus1", g, _speech(9202, FAST_MAX_LEN + 1), "the first generic-layout length",
                        paths=("generic", "general"), boundary=("fast", 1)))
    out.append(EdgeClip("len_fused_cap", g, _speech(9203, cap), "the longest clip of the fused kernel",
                        paths=("generic", "general"), boundary=("fused", 0)))
    out.append(EdgeClip("len_fused_cap_plus1", g, _speech(9204, cap + 1), "the first clip only the general kernel takes",
                        paths=("general",), boundary=("fused", 1)))
    return out


def _frames_clips():
    L, S = GROUPS["frames"]
    g = "frames"
    out = []
    # ---- VAD frame counts ----
    for nv in (1, 2, 9, 10, 11, 63, 64, 65, 127, 128, 129):
        n = L + (nv - 1) * S
        out.append(EdgeClip("nv%d" % nv, g, _speech(9300 + nv, n), "%d VAD frames" % nv, nv=nv, F=nv,
                            paths=PATHS if nv <= 128 else ("generic", "general"),
                            boundary=("fast", 0) if nv == 128 else None))
    for nv in (64, 65, 128):
        n = L + (nv - 1) * S
        tied = _tone(n, 44, 8000)  # period 44 divides S = 220: every full frame has the same samples
        out.append(EdgeClip("nv%d_tied" % nv, g, tied, "%d VAD frames of equal energy (all p90 keys equal)" % nv,
                            nv=nv, F=nv))
        x = tied.copy()
        for f in range(3, nv - 3, 3):  # one sample of a frame in three, +-1: equal high key halves
            x[f * S + 500] += 1 if f % 2 else -1
        out.append(EdgeClip("nv%d_tied_pm1" % nv, g, x, "%d VAD frames whose energies differ in their low bits" % nv,
                            nv=nv, F=nv))
    # ---- feature frame counts, endpoint detection off ----
    for F in (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129):
        paths = PATHS if F <= 128 else ("generic", "general")
        n = L + (F - 1) * S
        if not any(c.pcm.size == n for c in out):  # (the nv clips of the same length already end on a frame)
            out.append(EdgeClip("F%d_exact" % F, g, _speech(9500 + F, n), "%d feature frames, the last one full" % F,
                                nv=F, F=F, paths=paths))
        n = L + (F - 2) * S + 1 if F > 1 else L - 1
        out.append(EdgeClip("F%d_padded" % F, g, _speech(9700 + F, n), "%d feature frames, the last one zero-padded" % F,
                            nv=F - 1, F=F, paths=paths, boundary=("fast", 1) if F == 129 else None))
    return out


def _framelen_clips(g):
    x = _speech(9800, 12345)
    x[6000:6012] = NEG
    return [EdgeClip("speech_16000", g, _speech(9801, 16000), "ordinary clip at this frame length"),
            EdgeClip("speech_12345", g, _speech(9802, 12345), "odd length"),
            EdgeClip("speech_neg_run", g, x, "a 12-sample -32768 run", wrap_leads=tuple(range(8)))]


_CORPUS = None


def corpus():
    """The whole corpus, built once per process (list of EdgeClip; treat the arrays as read-only)."""
    global _CORPUS
    if _CORPUS is None:
        clips = _main_clips() + _frames_clips()
        for g in ("lcap", "lcap1", "lshift"):
            cs = _framelen_clips(g)
            if g == "lcap1":
                for c in cs:
                    c.paths = ("generic", "general")
            clips += cs
        for c in clips:
            c.pcm.setflags(write=False)
        names = [(c.group, c.name) for c in clips]
        assert len(set(names)) == len(names)
        _CORPUS = clips
    return _CORPUS


def group_clips(group, path):
    return [c for c in corpus() if c.group == group and path in c.paths]


def pack(clips, lead):
    """Clips back to back after `lead` junk samples, as test_gpu_position._pack: -> (pcm, offsets)."""
    parts = [np.full(lead, 1234, np.int16)] + [c.pcm for c in clips] + [np.zeros(16, np.int16)]
    off = np.zeros(len(clips) + 1, np.int64)
    off[0] = lead
    off[1:] = lead + np.cumsum([c.pcm.size for c in clips])
    return np.concatenate(parts), off
