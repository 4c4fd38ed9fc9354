"""Batched device API of the hot path (PyTorch-ROCm tensors in, tensors out).

This is what the reference's per-file loop becomes (experiments/run_experiments.py:78-111):
a batch of int16 clips resident in HBM goes through one fused HIP launch
(``dsp_extract_features``) and a 15-d feature matrix comes back, then
``knn_classify`` runs KNeighborsClassifier's exact k-NN + vote on the device.
"""
import numpy as np

from . import _hip

FEATURE_NAMES = ["%s_%s" % (f, s) for f in ("energy", "magnitude", "zcr")
                 for s in ("mean", "std", "max", "min", "median")]


def create_window(window_type, length):
    """src/audio_processing.py:278-296 -- host-side coefficients, exactly numpy's."""
    if window_type == "rectangular":
        return np.ones(length)
    if window_type == "hamming":
        return np.hamming(length)
    if window_type == "hanning":
        return np.hanning(length)
    raise ValueError("不支持的窗函数类型: %s" % window_type)


def _as_device(x, dtype, device):
    import torch
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype).contiguous()
    return torch.as_tensor(np.array(x, copy=True, order="C")).to(device=device, dtype=dtype).contiguous()


def _as_host(x, dtype=None):
    """x as a numpy array: a tensor is downloaded, a numpy array is returned as it is (no copy)."""
    return np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x, dtype=dtype)


class FeatureExtractor:
    """Reusable launch plan for ``dsp_extract_features`` (outputs preallocated per batch size).

    Parameters mirror process_audio_file (src/audio_processing.py:336-341) with frame sizes
    in samples, as the reference's callers pass them (experiments/run_experiments.py:90-99).
    """

    def __init__(self, frame_length, frame_shift, window_type="hamming", do_endpoint_detection=True,
                 energy_high_ratio=0.5, energy_low_ratio=0.1, zcr_threshold_ratio=1.5,
                 return_vad_lists=False, return_sequences=False, device=None):
        import torch
        self.device = device or _hip.require_device()
        self.L, self.S = int(frame_length), int(frame_shift)
        if self.L < 1 or self.S < 1:
            raise ValueError("frame_length and frame_shift must be positive")
        self.window_type = window_type
        self.window = torch.as_tensor(create_window(window_type, self.L), dtype=torch.float64).to(self.device)
        self.do_vad = bool(do_endpoint_detection)
        self.ratios = (float(energy_high_ratio), float(energy_low_ratio), float(zcr_threshold_ratio))
        self.return_vad_lists = return_vad_lists
        self.return_sequences = return_sequences
        self._bufs = {}

    def _queue_ws(self):
        """The zeroed DSP_QUEUE_WS_BYTES scratch of this extractor's launches on the CURRENT
        stream.  Launches on one stream are ordered, so they share one buffer (each launch leaves
        it zeroed); a launch on another stream -- including a HIP-graph capture, whose replays
        may overlap eager calls -- gets its own, so two launches can never claim chunks from the
        same counters."""
        import torch
        qs = self.__dict__.setdefault("_queues", {})
        key = torch.cuda.current_stream(self.device).cuda_stream
        q = qs.get(key)
        if q is None:
            q = qs[key] = torch.zeros(_hip.QUEUE_WS_BYTES // 4, dtype=torch.int32, device=self.device)
        return q

    def lds_bytes(self, max_len):
        return _hip.lib().dsp_extract_lds_bytes(int(max_len), self.L, self.S)

    def _outputs(self, B, max_len):
        import torch
        key = (B, max_len)
        if key not in self._bufs:
            d = self.device
            # one packed row per clip (DSP_OUT_ROW_WORDS int32 words: feat[15] as f32 bits, start,
            # end, n_frames, status), written by the kernels with out_stride = 19; the four result
            # arrays are strided views of it, and "rows" travels in one collective unpacked
            rows = torch.empty((B, _hip.OUT_ROW_WORDS), dtype=torch.int32, device=d)
            o = dict(rows=rows, feat=rows.view(torch.float32)[:, :15], start_end=rows[:, 15:17],
                     n_frames=rows[:, 17], status=rows[:, 18])
            if self.return_vad_lists:
                ld = max(1, (max_len - self.L) // self.S + 1) if max_len >= self.L else 1
                o["vad_energy"] = torch.zeros((B, ld), dtype=torch.float64, device=d)
                o["vad_zcr"] = torch.zeros((B, ld), dtype=torch.int32, device=d)
            if self.return_sequences:
                ld = 1 if max_len <= self.L else (max_len - self.L + self.S - 1) // self.S + 1
                o["seq"] = torch.zeros((B, ld, 3), dtype=torch.float32, device=d)
            self._bufs = {key: o}  # keep one shape alive
        return self._bufs[key]

    def fused_cap(self):
        """Longest clip (samples) the fused kernel's on-chip plan holds at this (L, S)."""
        if not hasattr(self, "_fcap"):
            lib, lo, hi = _hip.lib(), 0, 1 << 24
            while lo < hi:  # dsp_extract_lds_bytes is non-zero exactly for n <= cap
                mid = (lo + hi + 1) // 2
                if lib.dsp_extract_lds_bytes(mid, self.L, self.S) > 0:
                    lo = mid
                else:
                    hi = mid - 1
            self._fcap = lo
        return self._fcap

    def __call__(self, pcm, offsets=None, max_len=None):
        """pcm: int16 or int32 [B, N] (uniform clips) or packed 1-D with int64 offsets [B+1].

        int16 clips that fit the fused kernel's on-chip plan run in one fused launch; longer
        clips, and int32 samples (16-bit stereo channel sums), run on dsp_extract_general in the
        same stream order.  An explicit ``max_len`` caps the clips processed (longer ones report
        DSP_CLIP_TOO_LONG); without it, device-tensor offsets cost one host sync (the longest
        clip sizes the launch), so pass ``max_len`` to capture the call in a HIP graph.  Returns a
        dict of device tensors: feat [B,15] f32, start_end [B,2] i32, n_frames [B] i32, status
        [B] i32 -- strided views of ``rows`` [B,19] i32, each clip's packed 76-B record -- (+
        vad_energy/vad_zcr, seq when requested).  The tensors are reused by the next call with the
        same shape.
        """
        import torch
        d = self.device
        wide = str(getattr(pcm, "dtype", "")) in ("int32", "torch.int32")
        pcm = _as_device(pcm, torch.int32 if wide else torch.int16, d)
        if offsets is None:
            if pcm.dim() != 2:
                raise ValueError("1-D packed pcm needs offsets")
            B, N = pcm.shape
            key = ("uni", B, N)
            if key not in self._bufs:
                self._bufs[key] = torch.arange(B + 1, dtype=torch.int64, device=d) * N
            off = self._bufs[key]
            true_max = N
        else:
            if isinstance(offsets, np.ndarray) or not isinstance(offsets, torch.Tensor):
                lens = np.diff(np.asarray(offsets, dtype=np.int64))
                true_max = int(lens.max()) if lens.size else 1
            else:
                true_max = None
            off = _as_device(offsets, torch.int64, d)
            B = off.numel() - 1
            if true_max is None:
                true_max = int(torch.max(off[1:] - off[:-1]).item()) if B > 0 else 1
        if max_len is None:
            max_len = true_max
        pcm = pcm.reshape(-1)
        max_len = max(int(max_len), 1)
        out = self._outputs(B, max_len)
        hi, lo, zr = self.ratios
        ve, vz, ldv = out.get("vad_energy"), out.get("vad_zcr"), 0
        if ve is not None:
            ldv = ve.shape[1]
        sq, lds_ = out.get("seq"), 0
        if sq is not None:
            lds_ = sq.shape[1]
        args = (int(self.do_vad), hi, lo, zr, _hip.ptr(out["feat"]), _hip.ptr(out["start_end"]),
                _hip.ptr(out["n_frames"]), _hip.ptr(out["status"]), _hip.OUT_ROW_WORDS, _hip.ptr(ve),
                _hip.ptr(vz), ldv, _hip.ptr(sq), lds_)
        cap = 0 if wide else self.fused_cap()
        if not wide and B > 0 and cap > 0:
            # the clip-queue scratch: zeroed once, and every launch leaves it zeroed again (the
            # last workgroup out of each kernel resets its counters), so the launches of this
            # extractor on its stream reuse one buffer without a fill kernel per call
            queue = self._queue_ws()
            rc = _hip.lib().dsp_extract_features(
                _hip.ptr(pcm), _hip.ptr(off), B, min(max_len, cap), self.L, self.S,
                _hip.ptr(self.window), *args, _hip.ptr(queue), _hip.stream_handle(d))
            _hip.check(rc, "dsp_extract_features")
        if B > 0 and (wide or max_len > cap):
            # the clips the fused kernel cannot hold (longer than cap, or every clip of an int32
            # batch, or all of them when the fused plan holds none at this frame length): the
            # general kernel over the whole batch, its length window [cap + 1, max_len] selecting
            # them on the device -- no host round trip, so the call stays graph-capturable
            nbytes = _hip.lib().dsp_extract_general_workspace_bytes(B, max_len, self.L, self.S)
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=d)
            rc = _hip.lib().dsp_extract_general(
                _hip.ptr(pcm), 4 if wide else 2, _hip.ptr(off), None, B, cap, max_len, self.L, self.S,
                _hip.ptr(self.window), *args, _hip.ptr(ws), nbytes, _hip.stream_handle(d))
            _hip.check(rc, "dsp_extract_general")
            self._keep = ws  # stream-ordered use: the caching allocator reuses it only after the launch
        return out


def process_audio_batch(pcm, offsets=None, frame_length=1102, frame_shift=441, window_type="hamming",
                        do_endpoint_detection=True, energy_high_ratio=0.5, energy_low_ratio=0.1,
                        zcr_threshold_ratio=1.5, return_vad_lists=False, return_sequences=False,
                        max_len=None):
    """One-shot batched form of process_audio_file + extract_features_from_frames."""
    fx = FeatureExtractor(frame_length, frame_shift, window_type, do_endpoint_detection,
                          energy_high_ratio, energy_low_ratio, zcr_threshold_ratio,
                          return_vad_lists, return_sequences)
    return dict(fx(pcm, offsets, max_len))


class KnnIndex:
    """A reference set prepared for ``dsp_knn_classify`` -- KNeighborsClassifier.fit's side
    (src/models.py:52-55): the first query converts the rows for the screen into this index's
    workspace, and every later query against the same set skips that step (DSP_KNN_REF_READY).
    ``query`` is predict / kneighbors.  One query at a time per index (a workspace is a launch's
    scratch); the workspace grows to the largest query batch seen."""

    def __init__(self, ref, ref_labels, k, n_classes=None, with_pred=True):
        import torch
        self.device = _hip.require_device()
        self.ref = _as_device(ref, torch.float64, self.device)
        self.Nr, self.D = self.ref.shape
        self.k = int(k)
        self.labels = _as_device(ref_labels, torch.int32, self.device) if (ref_labels is not None and with_pred) else None
        self.n_classes = int(n_classes or 0)
        self._ws, self._ready = None, False

    def query(self, query, self_offset=-1, stats=None):
        """(idx int32 [Nq,k], dist float64 [Nq,k], pred int32 [Nq] or None); a dict passed as
        ``stats`` receives "fallbacks" (queries answered by the exhaustive fp64 scan; one host sync)."""
        import torch
        d, k = self.device, self.k
        q = _as_device(query, torch.float64, d)
        Nq = q.shape[0]
        ws_bytes = _hip.lib().dsp_knn_workspace_bytes(self.Nr, Nq, self.D, k)
        if ws_bytes == 0 and Nq > 0:
            raise ValueError("unsupported KNN shape (1 <= D <= 4096, 1 <= k <= 32)")
        if self._ws is None or self._ws.numel() < ws_bytes:
            self._ws, self._ready = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=d), False
        idx = torch.empty((Nq, k), dtype=torch.int32, device=d)
        dist = torch.empty((Nq, k), dtype=torch.float64, device=d)
        pred = torch.empty(Nq, dtype=torch.int32, device=d) if self.labels is not None else None
        if pred is not None and self.Nr == 0:
            pred.fill_(-1)  # an empty label array is a null pointer, which skips the vote: no candidate, no label
        flags = _hip.KNN_REF_READY if self._ready else 0
        rc = _hip.lib().dsp_knn_classify(_hip.ptr(self.ref), _hip.ptr(self.labels), self.Nr, _hip.ptr(q), Nq,
                                         self.D, k, int(self_offset), self.n_classes, _hip.ptr(idx),
                                         _hip.ptr(dist), _hip.ptr(pred), _hip.ptr(self._ws), self._ws.numel(),
                                         flags, _hip.stream_handle(d))
        _hip.check(rc, "dsp_knn_classify")
        self._ready = self._ready or (Nq > 0 and self.Nr > 0)
        if stats is not None and Nq > 0:
            off = _hip.lib().dsp_knn_workspace_fallbacks_offset(self.Nr, Nq, self.D, k)
            stats["fallbacks"] = int(self._ws[off:off + 4].view(torch.int32).item())
        return idx, dist, pred


def knn_classify(ref, ref_labels, query, k, self_offset=-1, n_classes=None, with_pred=True, stats=None):
    """Exact k-NN (KNeighborsClassifier semantics) on the device, one-shot (``KnnIndex`` keeps the
    prepared reference set across queries).

    ref [Nr, D] / query [Nq, D] float64 (cast if needed), ref_labels int [Nr].
    Returns (idx int32 [Nq,k], dist float64 [Nq,k], pred int32 [Nq] or None).  Where a query has
    fewer than k candidates idx is -1 and dist inf; with no candidate at all pred is -1.  A dict
    passed as ``stats`` receives "fallbacks": the queries answered by the exhaustive fp64 fallback
    (one host sync).

    The values must be finite (NaN and infinity are outside the contract, as for scikit-learn, and
    are not checked); any finite magnitude whose float64 squared distances are finite is exact.
    """
    return KnnIndex(ref, ref_labels, k, n_classes, with_pred).query(query, self_offset, stats)


def _dtw_operand(seqs, lengths, device, check_finite):
    """Padded sequences [N, T, F] and their lengths on the device as float64 / int32 (the
    extraction's float32 ``seq`` converts exactly).  Non-finite samples raise ValueError, as
    scikit-learn's estimators do (one host sync for a device tensor; check_finite=False skips it)."""
    import torch
    x = _as_device(seqs, torch.float64, device)
    if x.dim() != 3:
        raise ValueError("sequences must be padded to [N, T, F], got shape %s" % (tuple(x.shape),))
    n = _as_device(lengths, torch.int32, device).reshape(-1)
    if n.numel() != x.shape[0]:
        raise ValueError("%d lengths for %d sequences" % (n.numel(), x.shape[0]))
    if check_finite and x.numel() and not bool(torch.isfinite(x).all().item()):
        raise ValueError("Input sequences contain NaN or infinity")
    return x, n


def _dtw_window(window):
    return -1 if window is None or int(window) < 0 else int(window)


_DTW_SHAPE = "unsupported DTW shape (1 <= F <= 8, 1 <= T <= 1024)"


def _grown(ws, nbytes, unsupported, device):
    """The grow-only workspace of a call: ``nbytes`` is what its ``*_workspace_bytes`` function returned
    (0: the shape is outside the plan, ValueError(unsupported)); ``ws`` is kept when it is large enough."""
    import torch
    if nbytes == 0:
        raise ValueError(unsupported)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def dtw_pairwise(a, len_a, b, len_b, window=None, check_finite=True):
    """Dynamic time warping distances (include/dsp_audiorec.h: dsp_dtw_pairwise) between the padded
    sequences a [Nq, Tq, F] and b [Nr, Tr, F] with their lengths -> dist float64 [Nq, Nr] on the
    device.  ``window``: None / negative = unconstrained, else the Sakoe-Chiba band's half width."""
    import torch
    d = _hip.require_device()
    a, len_a = _dtw_operand(a, len_a, d, check_finite)
    b, len_b = _dtw_operand(b, len_b, d, check_finite)
    (Nq, Tq, F), (Nr, Tr, Fb) = a.shape, b.shape
    if F != Fb:
        raise ValueError("sequences of %d and %d feature channels" % (F, Fb))
    dist = torch.empty((Nq, Nr), dtype=torch.float64, device=d)
    if Nq == 0 or Nr == 0:
        return dist
    ws = _grown(None, _hip.lib().dsp_dtw_workspace_bytes(Nr, Nq, Tr, Tq, F, 1), _DTW_SHAPE, d)
    rc = _hip.lib().dsp_dtw_pairwise(_hip.ptr(a), _hip.ptr(len_a), Nq, Tq, _hip.ptr(b), _hip.ptr(len_b), Nr, Tr, F,
                                     _dtw_window(window), _hip.ptr(dist), _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
    _hip.check(rc, "dsp_dtw_pairwise")
    return dist


class DtwIndex:
    """A reference set of padded sequences uploaded once for ``dsp_dtw_knn`` (csrc/dtw.hip), the
    counterpart of ``KnnIndex`` under the DTW distance.  ``query`` is predict / kneighbors.  One
    query at a time per index; the workspace grows to the largest query batch seen."""

    def __init__(self, ref, len_ref, ref_labels, k, n_classes=None, window=None, check_finite=True):
        self.device = _hip.require_device()
        import torch
        self.ref, self.len_ref = _dtw_operand(ref, len_ref, self.device, check_finite)
        self.Nr, self.Tr, self.F = self.ref.shape
        self.k = int(k)
        self.labels = _as_device(ref_labels, torch.int32, self.device) if ref_labels is not None else None
        self.n_classes = int(n_classes or 0)
        self.window = _dtw_window(window)
        self._ws = None

    def query(self, seqs, lengths, self_offset=-1, check_finite=True):
        """(idx int32 [Nq,k], dist float64 [Nq,k], pred int32 [Nq] or None) of the padded query
        sequences [Nq, Tq, F]."""
        import torch
        d, k = self.device, self.k
        q, len_q = _dtw_operand(seqs, lengths, d, check_finite)
        Nq, Tq, F = q.shape
        if F != self.F:
            raise ValueError("queries of %d feature channels against references of %d" % (F, self.F))
        nbytes = _hip.lib().dsp_dtw_workspace_bytes(self.Nr, Nq, self.Tr, Tq, F, k)
        if nbytes == 0 and Nq > 0:
            raise ValueError("unsupported DTW shape (1 <= F <= 8, 1 <= T <= 1024, 1 <= k <= 32)")
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=d)
        idx = torch.empty((Nq, k), dtype=torch.int32, device=d)
        dist = torch.empty((Nq, k), dtype=torch.float64, device=d)
        pred = torch.empty(Nq, dtype=torch.int32, device=d) if self.labels is not None else None
        rc = _hip.lib().dsp_dtw_knn(_hip.ptr(self.ref), _hip.ptr(self.len_ref), _hip.ptr(self.labels), self.Nr,
                                    self.Tr, _hip.ptr(q), _hip.ptr(len_q), Nq, Tq, F, self.window, k,
                                    int(self_offset), self.n_classes, _hip.ptr(idx), _hip.ptr(dist), _hip.ptr(pred),
                                    _hip.ptr(self._ws), self._ws.numel(), _hip.stream_handle(d))
        _hip.check(rc, "dsp_dtw_knn")
        return idx, dist, pred


def _dtw_groups(groups, assign, Na, Nb):
    """The CSR pair list (group_start int32 [Na + 1], members int32 [P]) on the host, from the
    pair itself or from ``assign`` [Nb] (the a index of each b sequence, -1 to skip; a stable sort, so
    a group lists its members in ascending order)."""
    if (groups is None) == (assign is None):
        raise ValueError("pass either groups=(group_start, members) or assign")
    if assign is not None:
        assign = _as_host(assign).astype(np.int64).reshape(-1)
        if assign.size != Nb or (assign.size and (assign.min() < -1 or assign.max() >= Na)):
            raise ValueError("assign must hold one index in [-1, %d) per b sequence" % Na)
        members = np.flatnonzero(assign >= 0)
        members = members[np.argsort(assign[members], kind="stable")]
        start = np.concatenate([[0], np.cumsum(np.bincount(assign[members], minlength=Na))])
    else:
        start, members = (_as_host(g).astype(np.int64).reshape(-1) for g in groups)
        if start.size != Na + 1 or start[0] != 0 or (np.diff(start) < 0).any() or start[-1] != members.size:
            raise ValueError("group_start must be [Na + 1], non-decreasing from 0 to len(members)")
    return start.astype(np.int32), members.astype(np.int32)


def dtw_align(a, len_a, b, len_b, groups=None, assign=None, window=None, with_ranges=True, check_finite=True):
    """DTW alignment paths (include/dsp_audiorec.h: dsp_dtw_align) of the padded sequences
    b[members[p]] to a[c], the pairs given as the CSR ``groups=(group_start [Na + 1], members [P])`` or
    as ``assign`` [Nb].  Returns (dist float64 [P], lo, hi int32 [P, Ta] or None, group_start, members)
    on the device: frame i of a is matched to frames lo[i] .. hi[i] of b (-1 past a's length)."""
    import torch
    d = _hip.require_device()
    a, len_a = _dtw_operand(a, len_a, d, check_finite)
    b, len_b = _dtw_operand(b, len_b, d, check_finite)
    (Na, Ta, F), (Nb, Tb, Fb) = a.shape, b.shape
    if F != Fb:
        raise ValueError("sequences of %d and %d feature channels" % (F, Fb))
    start, members = _dtw_groups(groups, assign, Na, Nb)
    P = int(members.size)
    start, members = _as_device(start, torch.int32, d), _as_device(members, torch.int32, d)
    dist = torch.empty(P, dtype=torch.float64, device=d)
    lo = torch.empty((P, Ta), dtype=torch.int32, device=d) if with_ranges else None
    hi = torch.empty((P, Ta), dtype=torch.int32, device=d) if with_ranges else None
    if P > 0:
        ws = _grown(None, _hip.lib().dsp_dtw_align_workspace_bytes(Na, P, Ta, Tb, F), _DTW_SHAPE, d)
        rc = _hip.lib().dsp_dtw_align(_hip.ptr(a), _hip.ptr(len_a), Na, Ta, _hip.ptr(b), _hip.ptr(len_b), Nb, Tb, F,
                                      _dtw_window(window), _hip.ptr(start), _hip.ptr(members), P, _hip.ptr(dist),
                                      _hip.ptr(lo), _hip.ptr(hi), _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
        _hip.check(rc, "dsp_dtw_align")
    return dist, lo, hi, start, members


def dtw_path(x, y, window=None):
    """The warping path of one pair of [n, F] / [m, F] arrays: (distance, path int64 [L, 2]), the
    cells (i, j) ascending from (0, 0) to (n-1, m-1), expanded on the host from dsp_dtw_align's ranges."""
    x, y = (_as_host(v, np.float64) for v in (x, y))
    x, y = (v.reshape(-1, 1) if v.ndim == 1 else v for v in (x, y))
    if x.ndim != 2 or y.ndim != 2 or len(x) < 1 or len(y) < 1:
        raise ValueError("x and y must be non-empty [n, F] arrays")
    dist, lo, hi, _, _ = dtw_align(x[None], [len(x)], y[None], [len(y)], groups=([0, 1], [0]), window=window)
    lo, hi = lo[0].cpu().numpy().astype(np.int64), hi[0].cpu().numpy().astype(np.int64)
    count = hi - lo + 1
    i = np.repeat(np.arange(len(x)), count)
    j = np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count) + np.repeat(lo, count)
    return float(dist[0].item()), np.stack([i, j], axis=1)


class _PairListPlan:
    """What the two training updaters on a CSR pair list (csrc/csr_pairs.h) share: the padded sequences
    ``seqs`` [N, T, F] with ``len_s`` and the list ``start`` [C + 1], ``members`` [P] uploaded once, and one
    workspace that only grows, held across iterations."""

    def __init__(self, seqs, lengths, group_start, members, check_finite=True):
        import torch
        self.device = d = _hip.require_device()
        self.seqs, self.len_s = _dtw_operand(seqs, lengths, d, check_finite)
        self.N, self.T, self.F = self.seqs.shape
        self.C = len(group_start) - 1
        start, members = _dtw_groups((group_start, members), None, self.C, self.N)
        self.P = int(members.size)
        self.start, self.members = _as_device(start, torch.int32, d), _as_device(members, torch.int32, d)
        self._ws = None

    def _grow(self, nbytes, unsupported):
        self._ws = _grown(self._ws, nbytes, unsupported, self.device)
        return self._ws


class DbaUpdater(_PairListPlan):
    """The sequences of a DBA run uploaded once with their CSR class lists; ``update`` is one
    ``dsp_dtw_dba_update`` call for all templates: (new templates [C, Tt, F], inertia [C]) on the
    device."""

    def __init__(self, seqs, lengths, group_start, members, window=None, check_finite=True):
        super().__init__(seqs, lengths, group_start, members, check_finite)
        self.Ts, self.window = self.T, _dtw_window(window)

    def update(self, tmpl, len_t):
        import torch
        d = self.device
        tmpl, len_t = _dtw_operand(tmpl, len_t, d, False)
        C, Tt, F = tmpl.shape
        if C != self.C or F != self.F:
            raise ValueError("templates [%d, ., %d] for %d classes of %d channels" % (C, F, self.C, self.F))
        ws = self._grow(_hip.lib().dsp_dtw_align_workspace_bytes(C, self.P, Tt, self.Ts, F), _DTW_SHAPE)
        out = torch.empty_like(tmpl)
        inertia = torch.empty(C, dtype=torch.float64, device=d)
        rc = _hip.lib().dsp_dtw_dba_update(_hip.ptr(tmpl), _hip.ptr(len_t), C, Tt, _hip.ptr(self.seqs),
                                           _hip.ptr(self.len_s), self.N, self.Ts, F, self.window, _hip.ptr(self.start),
                                           _hip.ptr(self.members), self.P, _hip.ptr(out), _hip.ptr(inertia),
                                           _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
        _hip.check(rc, "dsp_dtw_dba_update")
        return out, inertia


def dtw_barycenter(seqs, lengths, init, n_iter=10, window=None, check_finite=True):
    """DTW barycentre averaging of the padded sequences [N, T, F] from the template ``init`` [L, F]:
    (template float64 [L, F], inertia float64 [iterations run]) as numpy arrays, inertia[t] the sum of
    squared DTW distances to the template that iteration t started from.  Stops early when an update
    returns the template bitwise unchanged; the result then equals running all ``n_iter``."""
    import torch
    init = _as_host(init, np.float64)
    init = init.reshape(-1, 1) if init.ndim == 1 else init
    N = len(lengths)
    up = DbaUpdater(seqs, lengths, [0, N], np.arange(N), window, check_finite)
    tmpl = _as_device(init[None], torch.float64, up.device)
    inertia = []
    for _ in range(int(n_iter)):
        new, inert = up.update(tmpl, [len(init)])
        inertia.append(float(inert[0].item()))
        same = bool(torch.equal(new.view(torch.int64), tmpl.view(torch.int64)))
        tmpl = new
        if same:
            break
    return tmpl[0].cpu().numpy(), np.array(inertia)


HMM_MAX_STATES = 32  # states of one model at most (csrc/hmm.hip keeps them in registers)


class _HmmSet:
    """What the left-to-right model sets share: ``_fields`` names the float64 arrays of the set in the order
    the C ABI takes them (the first one [C, Smax, .]); n_states int32 [C] follows them."""
    _fields = ()
    _dev = None

    @property
    def shape(self):
        return getattr(self, self._fields[0]).shape

    def on_device(self, device):
        """(the ``_fields`` arrays, n_states) as device tensors, uploaded once."""
        import torch
        if self._dev is None or self._dev[0].device != torch.device(device):
            self._dev = tuple(_as_device(getattr(self, f), torch.float64, device) for f in self._fields)
            self._dev += (_as_device(self.n_states, torch.int32, device),)
        return self._dev


def _hmm_p_stay(occ, n_valid, seen, trans_floor):
    """(occ - n_valid) / occ clamped to [trans_floor, 1 - trans_floor]; 0.5 where not ``seen``.  occ [C, Smax]:
    integer frame counts or float occupancies."""
    of = np.where(seen, occ, 2).astype(np.float64)
    p = (of - np.where(seen, n_valid[:, None], 1).astype(np.float64)) / of
    return np.minimum(np.maximum(p, trans_floor), 1.0 - trans_floor)


class HmmModelSet(_HmmSet):
    """C left-to-right Gaussian HMMs padded to Smax states, in the form ``dsp_hmm_score`` reads
    (include/dsp_audiorec.h): mean, var, w [C, Smax, F], g, stay, adv [C, Smax] float64 and n_states
    int32 [C], numpy arrays on the host.  This is the only place a logarithm is taken:
        w = 0.5 / var;  g = 0.5 * (log(2 pi var_0) + log(2 pi var_1) + ...)    channels in ascending order
        p_stay = (cnt - n_valid) / cnt, clamped to [trans_floor, 1 - trans_floor]
        stay = -log(p_stay);  adv = -log(1 - p_stay)
    Rows s >= n_states[c] are zeros.  A model with n_valid == 0 keeps ``prev``'s stay / adv (p_stay = 0.5
    without ``prev``)."""

    _fields = ("mean", "w", "g", "stay", "adv")

    def __init__(self, mean, var, cnt, n_valid, n_states, trans_floor=1e-3, prev=None):
        mean, var = (_as_host(v, np.float64) for v in (mean, var))
        cnt, n_valid, n_states = (_as_host(v).astype(np.int64) for v in (cnt, n_valid, n_states))
        if mean.ndim != 3 or var.shape != mean.shape or cnt.shape != mean.shape[:2]:
            raise ValueError("mean and var must be [C, Smax, F] and cnt [C, Smax]")
        C, Smax, _ = mean.shape
        if n_states.shape != (C,) or n_valid.shape != (C,) or Smax > HMM_MAX_STATES:
            raise ValueError("n_states and n_valid must be [C], Smax <= %d" % HMM_MAX_STATES)
        if C and (n_states.min() < 1 or n_states.max() > Smax):
            raise ValueError("n_states must lie in [1, %d]" % Smax)
        if not 0.0 < trans_floor < 0.5:
            raise ValueError("trans_floor must lie in (0, 0.5)")
        valid = np.arange(Smax)[None, :] < n_states[:, None]
        v = np.where(valid[:, :, None], var, 1.0)
        if not (np.isfinite(mean).all() and np.isfinite(v).all() and (v > 0).all()):
            raise ValueError("means must be finite and variances finite and positive")
        self.n_states = n_states.astype(np.int32)
        self.mean = np.where(valid[:, :, None], mean, 0.0)
        self.var = np.where(valid[:, :, None], var, 0.0)
        self.w = np.where(valid[:, :, None], 0.5 / v, 0.0)
        self.g = np.where(valid, 0.5 * np.cumsum(np.log((2.0 * np.pi) * v), axis=2)[:, :, -1], 0.0)
        seen = valid & (cnt > 0) & (n_valid[:, None] > 0)
        p = _hmm_p_stay(cnt, n_valid, seen, trans_floor)
        stay, adv = -np.log(p), -np.log(1.0 - p)
        if prev is not None:
            keep = (n_valid == 0)[:, None]
            stay, adv = np.where(keep, prev.stay, stay), np.where(keep, prev.adv, adv)
        self.stay, self.adv = np.where(valid, stay, 0.0), np.where(valid, adv, 0.0)


_HMM_SHAPE = "unsupported HMM shape (1 <= F <= 8, 1 <= T <= 1024, 1 <= Smax <= %d)" % HMM_MAX_STATES


def _hmm_model_args(models, F, device):
    C, Smax, Fm = models.shape
    if Fm != F:
        raise ValueError("sequences of %d feature channels against models of %d" % (F, Fm))
    return [_hip.ptr(t) for t in models.on_device(device)] + [C, Smax]


def hmm_score(models, seqs, lengths, with_labels=False, check_finite=True, _ws=None):
    """Viterbi scores (include/dsp_audiorec.h: dsp_hmm_score) of the padded sequences [N, T, F] under
    every model of the ``HmmModelSet``: (score float64 [N, C], the negative log-likelihood of the best
    state path, +inf where the sequence is shorter than the model; label int32 [N] or None: the
    smallest score's model, -1 when every score is +inf) on the device."""
    import torch
    d = _hip.require_device()
    x, n = _dtw_operand(seqs, lengths, d, check_finite)
    N, T, F = x.shape
    margs = _hmm_model_args(models, F, d)
    C, Smax = margs[-2:]
    score = torch.empty((N, C), dtype=torch.float64, device=d)
    label = torch.empty(N, dtype=torch.int32, device=d) if with_labels else None
    if N > 0:
        ws = _grown(_ws, _hip.lib().dsp_hmm_workspace_bytes(C, N, 0, T, F, Smax), _HMM_SHAPE, d)
        rc = _hip.lib().dsp_hmm_score(*margs, _hip.ptr(x), _hip.ptr(n), N, T, F, _hip.ptr(score), _hip.ptr(label),
                                      _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
        _hip.check(rc, "dsp_hmm_score")
    return score, label


class HmmUpdater(_PairListPlan):
    """The sequences of a Viterbi training run uploaded once with their CSR class lists (one group per
    model); the workspace is held across iterations.  ``align`` is one ``dsp_hmm_align`` call for all
    models, ``accumulate`` one ``dsp_hmm_accumulate`` call."""

    def _workspace(self, Smax):
        return self._grow(_hip.lib().dsp_hmm_workspace_bytes(self.C, self.N, self.P, self.T, self.F, Smax), _HMM_SHAPE)

    def align(self, models, with_seg=True):
        """(score float64 [P], seg int32 [P, Smax] or None) of every listed pair."""
        import torch
        d = self.device
        margs = _hmm_model_args(models, self.F, d)
        C, Smax = margs[-2:]
        if C != self.C:
            raise ValueError("%d models for %d groups" % (C, self.C))
        score = torch.empty(self.P, dtype=torch.float64, device=d)
        seg = torch.empty((self.P, Smax), dtype=torch.int32, device=d) if with_seg else None
        if self.P > 0 and C > 0:
            ws = self._workspace(Smax)
            rc = _hip.lib().dsp_hmm_align(*margs, _hip.ptr(self.seqs), _hip.ptr(self.len_s), self.N, self.T, self.F,
                                          _hip.ptr(self.start), _hip.ptr(self.members), self.P, _hip.ptr(score),
                                          _hip.ptr(seg), _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
            _hip.check(rc, "dsp_hmm_align")
        return score, seg

    def accumulate(self, mu_prev, var_prev, n_states, seg, score, var_floor=1e-3):
        """The re-estimation from a given segmentation: (mean, var float64 [C, Smax, F], cnt int32
        [C, Smax], n_valid int32 [C], total float64 [C]) on the device."""
        import torch
        d = self.device
        mu_prev, var_prev = _as_device(mu_prev, torch.float64, d), _as_device(var_prev, torch.float64, d)
        n_states, seg = _as_device(n_states, torch.int32, d).reshape(-1), _as_device(seg, torch.int32, d)
        score = _as_device(score, torch.float64, d).reshape(-1)
        if mu_prev.dim() != 3 or var_prev.shape != mu_prev.shape:
            raise ValueError("mu_prev and var_prev must be [C, Smax, F]")
        C, Smax, F = mu_prev.shape
        if C != self.C or F != self.F or n_states.numel() != C or tuple(seg.shape) != (self.P, Smax) or score.numel() != self.P:
            raise ValueError("models [%d, %d, %d], seg %s for %d groups, %d pairs of %d channels"
                             % (C, Smax, F, tuple(seg.shape), self.C, self.P, self.F))
        mean, var = torch.empty_like(mu_prev), torch.empty_like(var_prev)
        cnt = torch.empty((C, Smax), dtype=torch.int32, device=d)
        n_valid = torch.empty(C, dtype=torch.int32, device=d)
        total = torch.empty(C, dtype=torch.float64, device=d)
        if C > 0:
            ws = self._workspace(Smax)
            rc = _hip.lib().dsp_hmm_accumulate(_hip.ptr(mu_prev), _hip.ptr(var_prev), _hip.ptr(n_states), C, Smax,
                                               _hip.ptr(self.seqs), _hip.ptr(self.len_s), self.N, self.T, F,
                                               _hip.ptr(self.start), _hip.ptr(self.members), self.P, _hip.ptr(seg),
                                               _hip.ptr(score), float(var_floor), _hip.ptr(mean), _hip.ptr(var),
                                               _hip.ptr(cnt), _hip.ptr(n_valid), _hip.ptr(total), _hip.ptr(ws), ws.numel(),
                                               _hip.stream_handle(d))
            _hip.check(rc, "dsp_hmm_accumulate")
        return mean, var, cnt, n_valid, total


def hmm_align(models, seqs, lengths, groups=None, assign=None, with_seg=True, check_finite=True):
    """Viterbi state paths (include/dsp_audiorec.h: dsp_hmm_align) of the padded sequences
    seqs[members[p]] under model c, the pairs given as the CSR ``groups=(group_start [C + 1], members
    [P])`` or as ``assign`` [N] (the model of each sequence, -1 to skip).  Returns (score float64 [P], seg
    int32 [P, Smax] or None, group_start, members) on the device: seg[p, s] is the first frame of state
    s (-1 behind the model's states, and everywhere for a pair whose score is +inf)."""
    N = len(lengths)
    start, members = _dtw_groups(groups, assign, models.shape[0], N)
    up = HmmUpdater(seqs, lengths, start, members, check_finite)
    score, seg = up.align(models, with_seg)
    return score, seg, up.start, up.members


def hmm_uniform_segmentation(lengths, n_states, Smax):
    """The start of Viterbi training: state s of a pair with n frames and S states owns the frames
    floor(s n / S) .. floor((s + 1) n / S) - 1 (integer arithmetic) -> seg int32 [P, Smax]; -1 behind the
    model's states, and everywhere for a pair with n < S."""
    n, S = (np.asarray(v).astype(np.int64).reshape(-1) for v in (lengths, n_states))
    s = np.arange(int(Smax), dtype=np.int64)[None, :]
    seg = (s * n[:, None]) // np.maximum(S, 1)[:, None]
    return np.where((s < S[:, None]) & (n >= S)[:, None], seg, -1).astype(np.int32)


VQ_MAX_CODES = 256  # codewords of one codebook at most (csrc/vq.hip stages a codebook into 16 KiB of LDS)

_VQ_SHAPE = "unsupported VQ shape (1 <= F <= 8, 1 <= T <= 1024, 1 <= Kmax <= %d)" % VQ_MAX_CODES


def _vq_book_args(cb, n_codes, F, device):
    """(cb float64 [C, Kmax, F], n_codes int32 [C]) on the device and their C-ABI arguments."""
    import torch
    cb = _as_device(cb, torch.float64, device)
    n_codes = _as_device(n_codes, torch.int32, device).reshape(-1)
    if cb.dim() != 3 or n_codes.numel() != cb.shape[0]:
        raise ValueError("codebooks must be [C, Kmax, F] with one n_codes per codebook")
    if cb.shape[2] != F:
        raise ValueError("sequences of %d feature channels against codebooks of %d" % (F, cb.shape[2]))
    return cb, n_codes, [_hip.ptr(cb), _hip.ptr(n_codes), cb.shape[0], cb.shape[1]]


def vq_score(cb, n_codes, seqs, lengths, with_labels=False, check_finite=True):
    """Total quantisation distortions (include/dsp_audiorec.h: dsp_vq_score) of the padded sequences
    [N, T, F] under every codebook of cb [C, Kmax, F] with n_codes [C]: (score float64 [N, C], the sum over
    the sequence's frames of the squared distance to the nearest codeword; label int32 [N] or None: the
    smallest score's codebook, -1 when every score is +inf) on the device."""
    import torch
    d = _hip.require_device()
    x, n = _dtw_operand(seqs, lengths, d, check_finite)
    N, T, F = x.shape
    cb, n_codes, bargs = _vq_book_args(cb, n_codes, F, d)
    C, Kmax = bargs[-2:]
    score = torch.empty((N, C), dtype=torch.float64, device=d)
    label = torch.empty(N, dtype=torch.int32, device=d) if with_labels else None
    if N > 0:
        ws = _grown(None, _hip.lib().dsp_vq_workspace_bytes(C, N, 0, T, F, Kmax), _VQ_SHAPE, d)
        rc = _hip.lib().dsp_vq_score(*bargs, _hip.ptr(x), _hip.ptr(n), N, T, F, _hip.ptr(score), _hip.ptr(label),
                                     _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
        _hip.check(rc, "dsp_vq_score")
    return score, label


class VqUpdater(_PairListPlan):
    """The sequences of an LBG training run uploaded once with their CSR class lists (one group per
    codebook); the workspace is held across rounds.  ``assign`` is one ``dsp_vq_assign`` call for all
    codebooks, ``accumulate`` one ``dsp_vq_accumulate`` call."""

    def _workspace(self, Kmax):
        return self._grow(_hip.lib().dsp_vq_workspace_bytes(self.C, self.N, self.P, self.T, self.F, Kmax), _VQ_SHAPE)

    def assign(self, cb, n_codes, with_codes=True):
        """(dist float64 [P], code int32 [P, T] or None) of every listed pair."""
        import torch
        d = self.device
        cb, n_codes, bargs = _vq_book_args(cb, n_codes, self.F, d)
        C, Kmax = bargs[-2:]
        if C != self.C:
            raise ValueError("%d codebooks for %d groups" % (C, self.C))
        dist = torch.empty(self.P, dtype=torch.float64, device=d)
        code = torch.empty((self.P, self.T), dtype=torch.int32, device=d) if with_codes else None
        if self.P > 0 and C > 0:
            ws = self._workspace(Kmax)
            rc = _hip.lib().dsp_vq_assign(*bargs, _hip.ptr(self.seqs), _hip.ptr(self.len_s), self.N, self.T, self.F,
                                          _hip.ptr(self.start), _hip.ptr(self.members), self.P, _hip.ptr(dist),
                                          _hip.ptr(code), _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
            _hip.check(rc, "dsp_vq_assign")
        return dist, code

    def accumulate(self, cb_prev, n_codes, code, dist):
        """The Lloyd re-estimation from given codes: (centroid float64 [C, Kmax, F], cnt int32 [C, Kmax],
        n_valid int32 [C], total float64 [C]) on the device."""
        import torch
        d = self.device
        cb_prev, n_codes, bargs = _vq_book_args(cb_prev, n_codes, self.F, d)
        C, Kmax = bargs[-2:]
        code = _as_device(code, torch.int32, d)
        dist = _as_device(dist, torch.float64, d).reshape(-1)
        if C != self.C or tuple(code.shape) != (self.P, self.T) or dist.numel() != self.P:
            raise ValueError("codebooks [%d, %d, %d], code %s for %d groups, %d pairs of %d frames"
                             % (C, Kmax, self.F, tuple(code.shape), self.C, self.P, self.T))
        centroid = torch.empty_like(cb_prev)
        cnt = torch.empty((C, Kmax), dtype=torch.int32, device=d)
        n_valid = torch.empty(C, dtype=torch.int32, device=d)
        total = torch.empty(C, dtype=torch.float64, device=d)
        if C > 0:
            ws = self._workspace(Kmax)
            rc = _hip.lib().dsp_vq_accumulate(*bargs, _hip.ptr(self.seqs), _hip.ptr(self.len_s), self.N, self.T, self.F,
                                              _hip.ptr(self.start), _hip.ptr(self.members), self.P, _hip.ptr(code),
                                              _hip.ptr(dist), _hip.ptr(centroid), _hip.ptr(cnt), _hip.ptr(n_valid),
                                              _hip.ptr(total), _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
            _hip.check(rc, "dsp_vq_accumulate")
        return centroid, cnt, n_valid, total


def vq_assign(cb, n_codes, seqs, lengths, groups=None, assign=None, with_codes=True, check_finite=True):
    """Nearest codewords (include/dsp_audiorec.h: dsp_vq_assign) of the frames of the padded sequences
    seqs[members[p]] under codebook c, the pairs given as the CSR ``groups=(group_start [C + 1], members
    [P])`` or as ``assign`` [N] (the codebook of each sequence, -1 to skip).  Returns (dist float64 [P],
    code int32 [P, T] or None, group_start, members) on the device: code[p, t] is the codeword of frame t
    (-1 behind the sequence's frames, and everywhere for an invalid pair)."""
    N = len(lengths)
    start, members = _dtw_groups(groups, assign, len(_as_host(n_codes).reshape(-1)), N)
    up = VqUpdater(seqs, lengths, start, members, check_finite)
    dist, code = up.assign(cb, n_codes, with_codes)
    return dist, code, up.start, up.members


def vq_split(cb, eps):
    """The binary split of LBG training on cb [..., K, F] -> [..., 2 K, F]: codeword j becomes
    2 j = c + eps and 2 j + 1 = c - eps, elementwise (one rounded fp64 add / subtract each)."""
    cb = _as_host(cb, np.float64)
    eps = np.float64(eps)
    out = np.empty(cb.shape[:-2] + (2 * cb.shape[-2], cb.shape[-1]))
    out[..., 0::2, :] = cb + eps
    out[..., 1::2, :] = cb - eps
    return out


def vq_repair_empty(cb, cnt, n_codes, eps):
    """The empty-cell rule of LBG training on cb [C, Kmax, F] with the frame counts cnt [C, Kmax] of the
    round that produced it -> (cb, cnt) copies with, for each codebook and each empty cell j (cnt == 0,
    j < n_codes[c]) in ascending order: the donor is the cell with the largest cnt >= 2, ties to the
    smaller index; cb[j] = cb[donor] + eps, then cb[donor] = cb[donor] - eps, elementwise; for the rest of
    the pass the donor keeps cnt - cnt // 2 and j gets cnt // 2.  Without a donor the cell is left as it
    is."""
    cb = np.array(_as_host(cb, np.float64))
    cnt = np.array(_as_host(cnt)).astype(np.int64)
    n_codes = _as_host(n_codes).astype(np.int64).reshape(-1)
    eps = np.float64(eps)
    for c in range(cb.shape[0]):
        K = int(n_codes[c])
        for j in range(K):
            if cnt[c, j] != 0:
                continue
            donor = int(np.argmax(cnt[c, :K]))  # the first of the largest
            if cnt[c, donor] < 2:
                continue
            cb[c, j] = cb[c, donor] + eps
            cb[c, donor] = cb[c, donor] - eps
            cnt[c, j] = cnt[c, donor] // 2
            cnt[c, donor] -= cnt[c, j]
    return cb, cnt


DHMM_MAX_SYMBOLS = 256  # symbols of the shared alphabet at most (csrc/dhmm.hip stages a model's table into LDS)


def _dhmm_check(C, Smax, K, n_states):
    if n_states.shape != (C,) or not 1 <= Smax <= HMM_MAX_STATES or not 1 <= K <= DHMM_MAX_SYMBOLS:
        raise ValueError("n_states must be [C], 1 <= Smax <= %d, 1 <= K <= %d" % (HMM_MAX_STATES, DHMM_MAX_SYMBOLS))
    if C and (n_states.min() < 1 or n_states.max() > Smax):
        raise ValueError("n_states must lie in [1, %d]" % Smax)


def _dhmm_count_args(C, Smax, K, n_valid, n_states, alpha, trans_floor):
    """The checks both discrete sets make on what they are built from; (valid [C, Smax]: the states each
    model has, alpha as float64)."""
    _dhmm_check(C, Smax, K, n_states)
    if n_valid.shape != (C,):
        raise ValueError("n_valid must be [C]")
    if not (alpha > 0.0 and np.isfinite(alpha)):
        raise ValueError("alpha must be a positive number")
    if not 0.0 < trans_floor < 0.5:
        raise ValueError("trans_floor must lie in (0, 0.5)")
    return np.arange(Smax)[None, :] < n_states[:, None], np.float64(alpha)


def _dhmm_hand_built(table, stay, adv, n_states, names):
    """from_arrays' operands on the host, shapes checked: (table [C, Smax, K], stay, adv [C, Smax], n_states int32 [C])"""
    table, stay, adv = (np.array(_as_host(v, np.float64)) for v in (table, stay, adv))
    n_states = _as_host(n_states).astype(np.int64).reshape(-1)
    if table.ndim != 3 or stay.shape != table.shape[:2] or adv.shape != table.shape[:2]:
        raise ValueError("%s must be [C, Smax, K] and %s, %s [C, Smax]" % names)
    _dhmm_check(*table.shape, n_states)
    return table, stay, adv, n_states.astype(np.int32)


class DhmmModelSet(_HmmSet):
    """C left-to-right HMMs with discrete observations padded to Smax states over an alphabet of K
    symbols, in the form ``dsp_dhmm_score`` reads (include/dsp_audiorec.h): emit float64 [C, Smax, K],
    stay, adv float64 [C, Smax] and n_states int32 [C], numpy arrays on the host, built from the counts
    of ``dsp_dhmm_accumulate``.  This is the only place a logarithm is taken:
        emit = -log((cnt_emit + alpha) / (cnt + alpha * K))    in exactly that order, alpha * K one rounded product
        p_stay = (cnt - n_valid) / cnt, clamped to [trans_floor, 1 - trans_floor]
        stay = -log(p_stay);  adv = -log(1 - p_stay)
    ``alpha`` > 0, so a state nothing was counted for comes out uniform by itself.  Rows s >= n_states[c]
    are zeros.  A model with n_valid == 0 keeps ``prev``'s stay / adv (p_stay = 0.5 without ``prev``); its
    emissions come from its (all-zero) counts like any other's.  ``from_arrays`` takes a hand-built set."""

    _fields = ("emit", "stay", "adv")

    def __init__(self, cnt_emit, cnt, n_valid, n_states, alpha=0.5, trans_floor=1e-3, prev=None):
        cnt_emit, cnt, n_valid, n_states = (_as_host(v).astype(np.int64) for v in (cnt_emit, cnt, n_valid, n_states))
        if cnt_emit.ndim != 3 or cnt.shape != cnt_emit.shape[:2]:
            raise ValueError("cnt_emit must be [C, Smax, K] and cnt [C, Smax]")
        C, Smax, K = cnt_emit.shape
        valid, alpha = _dhmm_count_args(C, Smax, K, n_valid, n_states, alpha, trans_floor)
        den = cnt.astype(np.float64) + alpha * np.float64(K)
        emit = -np.log((cnt_emit.astype(np.float64) + alpha) / den[:, :, None])
        seen = valid & (cnt > 0) & (n_valid[:, None] > 0)
        p = _hmm_p_stay(cnt, n_valid, seen, trans_floor)
        stay, adv = -np.log(p), -np.log(1.0 - p)
        if prev is not None:
            keep = (n_valid == 0)[:, None]
            stay, adv = np.where(keep, prev.stay, stay), np.where(keep, prev.adv, adv)
        self.n_states = n_states.astype(np.int32)
        self.emit = np.where(valid[:, :, None], emit, 0.0)
        self.stay, self.adv = np.where(valid, stay, 0.0), np.where(valid, adv, 0.0)

    @classmethod
    def from_arrays(cls, emit, stay, adv, n_states):
        """A hand-built set: emit [C, Smax, K], stay, adv [C, Smax] as they are (finite or +inf, never NaN,
        never -inf), n_states [C]."""
        self = cls.__new__(cls)
        self.emit, self.stay, self.adv, self.n_states = _dhmm_hand_built(emit, stay, adv, n_states, ("emit", "stay", "adv"))
        for v in (self.emit, self.stay, self.adv):
            if np.isnan(v).any() or (v == -np.inf).any():
                raise ValueError("costs must be finite or +inf")
        return self


DHMM_MIN_PROB = 2.0 ** -300  # the smallest non-zero probability dsp_dhmm_forward reads (include/dsp_audiorec.h)


class DhmmProbSet(_HmmSet):
    """The model set of ``DhmmModelSet`` in the PROBABILITY domain, in the form ``dsp_dhmm_forward`` and
    ``dsp_dhmm_expect`` read (include/dsp_audiorec.h): pemit float64 [C, Smax, K], pstay, padv float64
    [C, Smax] and n_states int32 [C], numpy arrays on the host, built from the expected counts of
    ``dsp_dhmm_expect`` (or from the integer counts of ``dsp_dhmm_accumulate``, taken as they are):
        occ[c, s] = occ_emit[c, s, :] added sequentially in ascending k
        pemit = (occ_emit + alpha) / (occ + alpha * K)      alpha * K one rounded product
        pstay = (occ - n_valid) / occ, clamped to [trans_floor, 1 - trans_floor];  padv = 1.0 - pstay
    In a left-to-right model without skips every path leaves a state exactly once, so the expected advance
    count is n_valid: ``DhmmModelSet``'s formula with a real-valued occupancy.  pstay is 0.5 for a state
    nothing was seen in and for a model with n_valid == 0, which keeps ``prev``'s pstay when ``prev`` is
    given.  Rows s >= n_states[c] are zeros.  ``from_arrays`` takes a hand-built set; ``to_costs`` gives the
    ``DhmmModelSet`` of the same models, which feeds dhmm_score, dhmm_align and dhmm_decode unchanged."""

    _fields = ("pemit", "pstay", "padv")

    def __init__(self, occ_emit, n_valid, n_states, alpha=0.5, trans_floor=1e-3, prev=None):
        occ_emit = np.asarray(_as_host(occ_emit), np.float64)
        n_valid, n_states = (_as_host(v).astype(np.int64) for v in (n_valid, n_states))
        if occ_emit.ndim != 3:
            raise ValueError("occ_emit must be [C, Smax, K]")
        C, Smax, K = occ_emit.shape
        valid, alpha = _dhmm_count_args(C, Smax, K, n_valid, n_states, alpha, trans_floor)
        if not (np.isfinite(occ_emit).all() and (occ_emit >= 0.0).all()):
            raise ValueError("occ_emit must be finite and non-negative")
        occ = np.add.accumulate(occ_emit, axis=2)[:, :, -1]  # sequential, ascending k: np.sum adds pairwise
        pemit = (occ_emit + alpha) / (occ + alpha * np.float64(K))[:, :, None]
        seen = valid & (occ > 0.0) & (n_valid[:, None] > 0)
        p = _hmm_p_stay(occ, n_valid, seen, trans_floor)
        if prev is not None:
            p = np.where((n_valid == 0)[:, None], prev.pstay, p)
        self.n_states = n_states.astype(np.int32)
        self.pemit = np.where(valid[:, :, None], pemit, 0.0)
        self.pstay, self.padv = np.where(valid, p, 0.0), np.where(valid, 1.0 - p, 0.0)

    @classmethod
    def from_arrays(cls, pemit, pstay, padv, n_states):
        """A hand-built set: pemit [C, Smax, K], pstay, padv [C, Smax] as they are (every entry 0.0 or in
        [2^-300, 1], never NaN), n_states [C]."""
        self = cls.__new__(cls)
        self.pemit, self.pstay, self.padv, self.n_states = _dhmm_hand_built(pemit, pstay, padv, n_states,
                                                                            ("pemit", "pstay", "padv"))
        for v in (self.pemit, self.pstay, self.padv):
            if not ((v == 0.0) | ((v >= DHMM_MIN_PROB) & (v <= 1.0))).all():
                raise ValueError("probabilities must be 0.0 or lie in [2^-300, 1]")
        return self

    def to_costs(self):
        """The ``DhmmModelSet`` of the same models: -log p entry by entry, +inf for 0.0 (rows s >= n_states[c]
        stay zeros)."""
        valid = np.arange(self.shape[1])[None, :] < self.n_states[:, None]
        with np.errstate(divide="ignore"):
            emit, stay, adv = (-np.log(v) for v in (self.pemit, self.pstay, self.padv))
        return DhmmModelSet.from_arrays(np.where(valid[:, :, None], emit, 0.0), np.where(valid, stay, 0.0),
                                        np.where(valid, adv, 0.0), self.n_states)


_DHMM_SHAPE = ("unsupported discrete HMM shape (1 <= T <= 1024, 1 <= Smax <= %d, 1 <= K <= %d)"
               % (HMM_MAX_STATES, DHMM_MAX_SYMBOLS))


def _dhmm_operand(sym, lengths, device):
    """Symbol rows [N, T] and their lengths on the device as int32."""
    import torch
    s = _as_device(sym, torch.int32, device)
    if s.dim() != 2:
        raise ValueError("symbols must be padded to [N, T], got shape %s" % (tuple(s.shape),))
    n = _as_device(lengths, torch.int32, device).reshape(-1)
    if n.numel() != s.shape[0]:
        raise ValueError("%d lengths for %d symbol rows" % (n.numel(), s.shape[0]))
    return s.contiguous(), n


def _dhmm_model_args(models, device):
    C, Smax, K = models.shape
    return [_hip.ptr(t) for t in models.on_device(device)] + [C, Smax, K]


def dhmm_score(models, sym, lengths, with_labels=False, _ws=None):
    """Viterbi scores (include/dsp_audiorec.h: dsp_dhmm_score) of the symbol rows sym int32 [N, T] under
    every model of the ``DhmmModelSet``: (score float64 [N, C], +inf where the sequence is shorter than
    the model or holds a symbol outside the alphabet; label int32 [N] or None: the smallest score's model,
    -1 when every score is +inf) on the device."""
    import torch
    d = _hip.require_device()
    s, n = _dhmm_operand(sym, lengths, d)
    N, T = s.shape
    margs = _dhmm_model_args(models, d)
    C, Smax, K = margs[-3:]
    score = torch.empty((N, C), dtype=torch.float64, device=d)
    label = torch.empty(N, dtype=torch.int32, device=d) if with_labels else None
    if N > 0:
        ws = _grown(_ws, _hip.lib().dsp_dhmm_workspace_bytes(C, N, 0, T, Smax, K), _DHMM_SHAPE, d)
        rc = _hip.lib().dsp_dhmm_score(*margs, _hip.ptr(s), _hip.ptr(n), N, T, _hip.ptr(score), _hip.ptr(label),
                                       _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
        _hip.check(rc, "dsp_dhmm_score")
    return score, label


def dhmm_forward(models, sym, lengths, with_labels=False, _ws=None):
    """Forward likelihoods (include/dsp_audiorec.h: dsp_dhmm_forward) of the symbol rows sym int32 [N, T]
    under every model of the ``DhmmProbSet``: (mant float64 [N, C], expo int32 [N, C][, label int32 [N]]) on
    the device.  The likelihood is mant * 2^expo, mant in [0.5, 1), or (0.0, 0) where it is zero: a sequence
    shorter than the model, or one that holds a symbol outside the alphabet.  label: the model of the largest
    likelihood, -1 when every likelihood is zero.  ``dhmm_nll`` turns the pairs into negative logs."""
    import torch
    d = _hip.require_device()
    s, n = _dhmm_operand(sym, lengths, d)
    N, T = s.shape
    margs = _dhmm_model_args(models, d)
    C, Smax, K = margs[-3:]
    mant = torch.empty((N, C), dtype=torch.float64, device=d)
    expo = torch.empty((N, C), dtype=torch.int32, device=d)
    label = torch.empty(N, dtype=torch.int32, device=d) if with_labels else None
    if N > 0:
        ws = _grown(_ws, _hip.lib().dsp_dhmm_fb_workspace_bytes(C, N, 0, T, Smax, K), _DHMM_SHAPE, d)
        rc = _hip.lib().dsp_dhmm_forward(*margs, _hip.ptr(s), _hip.ptr(n), N, T, _hip.ptr(mant), _hip.ptr(expo),
                                         _hip.ptr(label), _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
        _hip.check(rc, "dsp_dhmm_forward")
    return (mant, expo, label) if with_labels else (mant, expo)


def dhmm_nll(mant, expo):
    """-(log(mant) + expo * log(2.0)) of ``dhmm_forward``'s pairs as a float64 numpy array, +inf where mant
    == 0: the only logarithm of the forward path, taken on the host."""
    mant, expo = np.asarray(_as_host(mant), np.float64), np.asarray(_as_host(expo)).astype(np.float64)
    zero = mant == 0.0
    return np.where(zero, np.inf, -(np.log(np.where(zero, 1.0, mant)) + expo * np.log(2.0)))


class DhmmUpdater(_PairListPlan):
    """The symbol rows of a Viterbi training run uploaded once with their CSR class lists (one group per
    model): the plan's ``seqs`` is the int32 [N, T] tensor; the workspace is held across iterations.
    ``align`` is one ``dsp_dhmm_align`` call for all models, ``accumulate`` one ``dsp_dhmm_accumulate`` call."""

    def __init__(self, sym, lengths, group_start, members):
        import torch
        self.device = d = _hip.require_device()
        self.seqs, self.len_s = _dhmm_operand(sym, lengths, d)
        self.N, self.T = self.seqs.shape
        self.C = len(group_start) - 1
        start, members = _dtw_groups((group_start, members), None, self.C, self.N)
        self.P = int(members.size)
        self.start, self.members = _as_device(start, torch.int32, d), _as_device(members, torch.int32, d)
        self._ws = self._fb_ws = None  # dsp_dhmm_workspace_bytes and dsp_dhmm_fb_workspace_bytes: each only grows

    def _workspace(self, Smax, K):
        return self._grow(_hip.lib().dsp_dhmm_workspace_bytes(self.C, self.N, self.P, self.T, Smax, K), _DHMM_SHAPE)

    def align(self, models, with_seg=True):
        """(score float64 [P], seg int32 [P, Smax] or None) of every listed pair."""
        import torch
        d = self.device
        margs = _dhmm_model_args(models, d)
        C, Smax, K = margs[-3:]
        if C != self.C:
            raise ValueError("%d models for %d groups" % (C, self.C))
        score = torch.empty(self.P, dtype=torch.float64, device=d)
        seg = torch.empty((self.P, Smax), dtype=torch.int32, device=d) if with_seg else None
        if self.P > 0 and C > 0:
            ws = self._workspace(Smax, K)
            rc = _hip.lib().dsp_dhmm_align(*margs, _hip.ptr(self.seqs), _hip.ptr(self.len_s), self.N, self.T,
                                           _hip.ptr(self.start), _hip.ptr(self.members), self.P, _hip.ptr(score),
                                           _hip.ptr(seg), _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
            _hip.check(rc, "dsp_dhmm_align")
        return score, seg

    def accumulate(self, n_states, K, seg, score):
        """The re-estimation from a given segmentation: (cnt_emit int32 [C, Smax, K], cnt int32 [C, Smax],
        n_valid int32 [C], total float64 [C]) on the device."""
        import torch
        d = self.device
        n_states, seg = _as_device(n_states, torch.int32, d).reshape(-1), _as_device(seg, torch.int32, d)
        score = _as_device(score, torch.float64, d).reshape(-1)
        C, K = self.C, int(K)
        if seg.dim() != 2 or n_states.numel() != C or seg.shape[0] != self.P or score.numel() != self.P:
            raise ValueError("%d n_states, seg %s for %d groups, %d pairs" % (n_states.numel(), tuple(seg.shape), C, self.P))
        Smax = seg.shape[1]
        cnt_emit = torch.empty((C, Smax, K), dtype=torch.int32, device=d)
        cnt = torch.empty((C, Smax), dtype=torch.int32, device=d)
        n_valid = torch.empty(C, dtype=torch.int32, device=d)
        total = torch.empty(C, dtype=torch.float64, device=d)
        if C > 0:
            ws = self._workspace(Smax, K)
            rc = _hip.lib().dsp_dhmm_accumulate(_hip.ptr(n_states), C, Smax, K, _hip.ptr(self.seqs), _hip.ptr(self.len_s),
                                                self.N, self.T, _hip.ptr(self.start), _hip.ptr(self.members), self.P,
                                                _hip.ptr(seg.contiguous()), _hip.ptr(score), _hip.ptr(cnt_emit), _hip.ptr(cnt),
                                                _hip.ptr(n_valid), _hip.ptr(total), _hip.ptr(ws), ws.numel(),
                                                _hip.stream_handle(d))
            _hip.check(rc, "dsp_dhmm_accumulate")
        return cnt_emit, cnt, n_valid, total

    def expect(self, models, with_gamma=False):
        """The forward-backward pass of every listed pair under the ``DhmmProbSet`` (one ``dsp_dhmm_expect``
        call): (mant float64 [P], expo int32 [P], occ_emit float64 [C, Smax, K], n_valid int32 [C][, gamma
        float64 [P, T, Smax]]) on the device."""
        import torch
        d = self.device
        margs = _dhmm_model_args(models, d)
        C, Smax, K = margs[-3:]
        if C != self.C:
            raise ValueError("%d models for %d groups" % (C, self.C))
        mant = torch.zeros(self.P, dtype=torch.float64, device=d)
        expo = torch.zeros(self.P, dtype=torch.int32, device=d)
        occ_emit = torch.empty((C, Smax, K), dtype=torch.float64, device=d)  # zeroed by the call itself
        n_valid = torch.empty(C, dtype=torch.int32, device=d)
        gamma = torch.empty((self.P, self.T, Smax), dtype=torch.float64, device=d) if with_gamma else None
        if C > 0:
            nbytes = _hip.lib().dsp_dhmm_fb_workspace_bytes(C, self.N, self.P, self.T, Smax, K)
            ws = self._fb_ws = _grown(self._fb_ws, nbytes, _DHMM_SHAPE, d)
            rc = _hip.lib().dsp_dhmm_expect(*margs, _hip.ptr(self.seqs), _hip.ptr(self.len_s), self.N, self.T,
                                            _hip.ptr(self.start), _hip.ptr(self.members), self.P, _hip.ptr(mant),
                                            _hip.ptr(expo), _hip.ptr(gamma), _hip.ptr(occ_emit), _hip.ptr(n_valid),
                                            _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
            _hip.check(rc, "dsp_dhmm_expect")
        out = (mant, expo, occ_emit, n_valid)
        return out + (gamma,) if with_gamma else out


def dhmm_posterior(models, sym, lengths, groups=None, assign=None):
    """State posteriors (include/dsp_audiorec.h: dsp_dhmm_expect) of the symbol rows sym[members[p]] under
    model c of the ``DhmmProbSet``, the pairs given as in ``dhmm_align``.  Returns (gamma float64 [P, T, Smax],
    group_start, members) on the device: gamma[p, t, s] the probability of state s at frame t given the whole
    sequence and the forced start and end, zeros behind the sequence's frames and the model's states and
    everywhere for a pair that is not valid."""
    N = len(lengths)
    start, members = _dtw_groups(groups, assign, models.shape[0], N)
    up = DhmmUpdater(sym, lengths, start, members)
    return up.expect(models, with_gamma=True)[4], up.start, up.members


def dhmm_align(models, sym, lengths, groups=None, assign=None, with_seg=True):
    """Viterbi state paths (include/dsp_audiorec.h: dsp_dhmm_align) of the symbol rows sym[members[p]]
    under model c, the pairs given as the CSR ``groups=(group_start [C + 1], members [P])`` or as ``assign``
    [N] (the model of each sequence, -1 to skip).  Returns (score float64 [P], seg int32 [P, Smax] or None,
    group_start, members) on the device, seg as ``hmm_align``'s."""
    N = len(lengths)
    start, members = _dtw_groups(groups, assign, models.shape[0], N)
    up = DhmmUpdater(sym, lengths, start, members)
    score, seg = up.align(models, with_seg)
    return score, seg, up.start, up.members


DHMM_DECODE_MAX_MODELS = 64  # word models of a decoding loop at most (csrc/dhmm_decode.hip: a lane per model)


def dhmm_decode(models, sym, lengths, enter=None, max_words=None):
    """Connected-word decoding (include/dsp_audiorec.h: dsp_dhmm_decode): the one-pass Viterbi of the
    symbol rows sym int32 [N, T] over a loop of the models of the ``DhmmModelSet`` (at most
    ``DHMM_DECODE_MAX_MODELS``).  ``enter``: the cost of starting a word, None (0.0), a scalar or one value
    per model, finite or +inf.  ``max_words``: the words kept per utterance, T when None.  Returns (score
    float64 [N], n_words int32 [N], words int32 [N, max_words], start int32 [N, max_words], cum float64
    [N, max_words]) on the device; -1 (cum: +inf) behind an utterance's words."""
    import torch
    d = _hip.require_device()
    s, n = _dhmm_operand(sym, lengths, d)
    N, T = s.shape
    margs = _dhmm_model_args(models, d)
    C, Smax, K = margs[-3:]
    if not 1 <= C <= DHMM_DECODE_MAX_MODELS:
        raise ValueError("a decoding loop takes 1 .. %d word models, got %d" % (DHMM_DECODE_MAX_MODELS, C))
    if T < 1:
        raise ValueError(_DHMM_SHAPE)
    max_words = T if max_words is None else int(max_words)
    if not 1 <= max_words <= T:
        raise ValueError("max_words must lie in [1, T = %d]" % T)
    cost = _dhmm_enter(enter, C, d)
    score = torch.empty(N, dtype=torch.float64, device=d)
    n_words = torch.empty(N, dtype=torch.int32, device=d)
    words = torch.empty((N, max_words), dtype=torch.int32, device=d)
    start = torch.empty((N, max_words), dtype=torch.int32, device=d)
    cum = torch.empty((N, max_words), dtype=torch.float64, device=d)
    if N > 0:
        ws = _grown(None, _hip.lib().dsp_dhmm_decode_workspace_bytes(C, N, T, Smax, K), _DHMM_SHAPE, d)
        rc = _hip.lib().dsp_dhmm_decode(*margs[:4], _hip.ptr(cost), C, Smax, K, _hip.ptr(s), _hip.ptr(n), N, T, max_words,
                                        _hip.ptr(score), _hip.ptr(n_words), _hip.ptr(words), _hip.ptr(start), _hip.ptr(cum),
                                        _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
        _hip.check(rc, "dsp_dhmm_decode")
    return score, n_words, words, start, cum


def _dhmm_costs(cost, shape, name, device):
    """A grammar's cost array on the device (float64, finite or +inf), or None."""
    import torch
    if cost is None:
        return None
    cost = np.ascontiguousarray(np.asarray(_as_host(cost), np.float64))
    if cost.shape != shape:
        raise ValueError("%s must have shape %s, got %s" % (name, shape, cost.shape))
    if np.isnan(cost).any() or (cost == -np.inf).any():
        raise ValueError("%s must be finite or +inf" % name)
    return _as_device(cost, torch.float64, device)


def dhmm_decode_grammar(models, sym, lengths, enter, pair, leave, max_words=None):
    """Connected-word decoding under a word-pair grammar (include/dsp_audiorec.h: dsp_dhmm_decode_grammar):
    ``dhmm_decode``'s one-pass Viterbi with the cost of a word change depending on the word before.  ``enter``
    float64 [C]: the cost of starting the utterance with each word, None for 0.0; ``pair`` float64 [C, C]:
    pair[p, c] the cost of word c following word p, any word penalty included; ``leave`` float64 [C]: the cost of
    ending on each word, None for 0.0; all finite or +inf, +inf forbids.  ``max_words``: the words kept per
    utterance, T when None.  Returns (score float64 [N], n_words int32 [N], words int32 [N, max_words], start
    int32 [N, max_words]) on the device; -1 behind an utterance's words.  There is no ``cum``."""
    import torch
    d = _hip.require_device()
    s, n = _dhmm_operand(sym, lengths, d)
    N, T = s.shape
    margs = _dhmm_model_args(models, d)
    C, Smax, K = margs[-3:]
    if not 1 <= C <= DHMM_DECODE_MAX_MODELS:
        raise ValueError("a decoding loop takes 1 .. %d word models, got %d" % (DHMM_DECODE_MAX_MODELS, C))
    if T < 1:
        raise ValueError(_DHMM_SHAPE)
    max_words = T if max_words is None else int(max_words)
    if not 1 <= max_words <= T:
        raise ValueError("max_words must lie in [1, T = %d]" % T)
    if pair is None:
        raise ValueError("a word-pair grammar needs pair [C, C]")
    costs = [_dhmm_costs(enter, (C,), "enter", d), _dhmm_costs(pair, (C, C), "pair", d), _dhmm_costs(leave, (C,), "leave", d)]
    score = torch.empty(N, dtype=torch.float64, device=d)
    n_words = torch.empty(N, dtype=torch.int32, device=d)
    words = torch.empty((N, max_words), dtype=torch.int32, device=d)
    start = torch.empty((N, max_words), dtype=torch.int32, device=d)
    if N > 0:
        ws = _grown(None, _hip.lib().dsp_dhmm_decode_grammar_workspace_bytes(C, N, T, Smax, K), _DHMM_SHAPE, d)
        rc = _hip.lib().dsp_dhmm_decode_grammar(*margs[:4], *[_hip.ptr(c) for c in costs], C, Smax, K, _hip.ptr(s), _hip.ptr(n),
                                                N, T, max_words, _hip.ptr(score), _hip.ptr(n_words), _hip.ptr(words),
                                                _hip.ptr(start), _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
        _hip.check(rc, "dsp_dhmm_decode_grammar")
    return score, n_words, words, start


DHMM_FORCE_MAX_WORDS = 64  # words of one transcript at most (csrc/dhmm_force.hip: a lane per transcript position)


def _dhmm_transcripts(transcripts, n_trans, N):
    """(trans int32 [N, Wmax], n_trans int32 [N]) on the host from a list of index sequences, or from a padded
    [N, Wmax] array with its word counts; 1 <= Wmax <= ``DHMM_FORCE_MAX_WORDS``."""
    if n_trans is None:
        rows = [np.asarray(_as_host(r)).astype(np.int64).reshape(-1) for r in transcripts]
        n_trans = np.array([len(r) for r in rows], np.int32)
        trans = np.full((len(rows), max(1, int(n_trans.max()) if len(rows) else 1)), -1, np.int32)
        for i, r in enumerate(rows):
            trans[i, :len(r)] = r
    else:
        trans = np.ascontiguousarray(_as_host(transcripts).astype(np.int32))
        n_trans = _as_host(n_trans).astype(np.int32).reshape(-1)
        if trans.ndim != 2:
            raise ValueError("padded transcripts must be [N, Wmax], got shape %s" % (trans.shape,))
    if trans.shape[0] != N or len(n_trans) != N:
        raise ValueError("%d transcripts and %d word counts for %d utterances" % (trans.shape[0], len(n_trans), N))
    if not 1 <= trans.shape[1] <= DHMM_FORCE_MAX_WORDS:
        raise ValueError("a transcript holds 1 .. %d words, got Wmax = %d" % (DHMM_FORCE_MAX_WORDS, trans.shape[1]))
    return trans, n_trans


def _dhmm_enter(enter, C, device):
    """The entry costs of ``dhmm_decode`` and ``dhmm_force_align`` on the device, or None (all 0.0)."""
    import torch
    if enter is None:
        return None
    cost = np.array(np.broadcast_to(np.asarray(_as_host(enter), np.float64), (C,)))
    if np.isnan(cost).any() or (cost == -np.inf).any():
        raise ValueError("enter must be finite or +inf")
    return _as_device(cost, torch.float64, device)


def dhmm_flat_segmentation(lengths, trans, n_trans, n_states, Smax):
    """The flat start of embedded training (host only): an utterance of n frames against the chain of its
    transcript's J = S_0 + S_1 + ... concatenated states; chain state j begins at frame floor(j n / J) --
    ``hmm_uniform_segmentation``'s rule on the chain.  Returns seg int32 [N, Wmax, Smax]: -1 behind each word's
    states and behind the transcript, and everywhere when n < J or the transcript is invalid (a word count
    outside 1 .. Wmax, an index outside the set, a model with n_states outside 1 .. Smax)."""
    n = np.asarray(lengths).astype(np.int64).reshape(-1)
    S_all = np.asarray(n_states).astype(np.int64).reshape(-1)
    trans, L = _dhmm_transcripts(trans, n_trans, len(n))
    trans, L = trans.astype(np.int64), L.astype(np.int64)
    N, Wmax = trans.shape
    Smax = int(Smax)
    inside = np.arange(Wmax)[None, :] < L[:, None]
    wok = (trans >= 0) & (trans < len(S_all))
    S = np.where(inside & wok, S_all[np.where(wok, trans, 0)], 0)  # [N, Wmax], 0 behind the transcript
    ok = (L >= 1) & (L <= Wmax) & ~(inside & (~wok | (S < 1) | (S > Smax))).any(axis=1)
    S = np.where(ok[:, None], np.minimum(S, Smax), 0)
    J = S.sum(axis=1)
    ok &= n >= J
    j = (np.cumsum(S, axis=1) - S)[:, :, None] + np.arange(Smax)[None, None, :]  # the chain index of (i, s)
    seg = (j * n[:, None, None]) // np.maximum(J, 1)[:, None, None]
    keep = ok[:, None, None] & (np.arange(Smax)[None, None, :] < S[:, :, None])
    return np.where(keep, seg, -1).astype(np.int32)


class DhmmForceUpdater:
    """The symbol rows of an embedded training run uploaded once with their transcripts (trans [N, Wmax],
    n_trans [N], or a list of index sequences with ``n_trans=None``); one workspace that only grows is held
    across the rounds.  ``align`` is one ``dsp_dhmm_force_align`` call, ``accumulate`` one
    ``dsp_dhmm_force_accumulate`` call (include/dsp_audiorec.h, csrc/dhmm_force.hip)."""

    def __init__(self, sym, lengths, trans, n_trans=None):
        import torch
        self.device = d = _hip.require_device()
        self.seqs, self.len_s = _dhmm_operand(sym, lengths, d)
        self.N, self.T = self.seqs.shape
        trans, n_trans = _dhmm_transcripts(trans, n_trans, self.N)
        self.Wmax = trans.shape[1]
        self.trans, self.n_trans = _as_device(trans, torch.int32, d), _as_device(n_trans, torch.int32, d)
        self._ws = None

    def _workspace(self, C, Smax, K):
        nbytes = _hip.lib().dsp_dhmm_force_workspace_bytes(C, self.N, self.T, self.Wmax, Smax, K)
        self._ws = _grown(self._ws, nbytes, _DHMM_FORCE_SHAPE, self.device)
        return self._ws

    def align(self, models, enter=None, with_seg=True):
        """(score float64 [N], seg int32 [N, Wmax, Smax] or None) of every utterance against its transcript."""
        import torch
        d = self.device
        margs = _dhmm_model_args(models, d)
        C, Smax, K = margs[-3:]
        cost = _dhmm_enter(enter, C, d)
        score = torch.empty(self.N, dtype=torch.float64, device=d)
        seg = torch.empty((self.N, self.Wmax, Smax), dtype=torch.int32, device=d) if with_seg else None
        if self.N > 0:
            ws = self._workspace(C, Smax, K)
            rc = _hip.lib().dsp_dhmm_force_align(*margs[:4], _hip.ptr(cost), C, Smax, K, _hip.ptr(self.seqs),
                                                 _hip.ptr(self.len_s), self.N, self.T, _hip.ptr(self.trans),
                                                 _hip.ptr(self.n_trans), self.Wmax, _hip.ptr(score), _hip.ptr(seg),
                                                 _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
            _hip.check(rc, "dsp_dhmm_force_align")
        return score, seg

    def accumulate(self, n_states, K, seg):
        """The embedded re-estimation from a given segmentation: (cnt_emit int32 [C, Smax, K], cnt int32
        [C, Smax], n_valid int32 [C], valid int32 [N]) on the device."""
        import torch
        d = self.device
        n_states, seg = _as_device(n_states, torch.int32, d).reshape(-1), _as_device(seg, torch.int32, d)
        C, K = n_states.numel(), int(K)
        if seg.dim() != 3 or seg.shape[0] != self.N or seg.shape[1] != self.Wmax:
            raise ValueError("seg %s for %d utterances of %d words at most" % (tuple(seg.shape), self.N, self.Wmax))
        Smax = seg.shape[2]
        cnt_emit = torch.empty((C, Smax, K), dtype=torch.int32, device=d)  # zeroed by the call itself
        cnt = torch.empty((C, Smax), dtype=torch.int32, device=d)
        n_valid = torch.empty(C, dtype=torch.int32, device=d)
        valid = torch.empty(self.N, dtype=torch.int32, device=d)
        ws = self._workspace(C, Smax, K)
        rc = _hip.lib().dsp_dhmm_force_accumulate(_hip.ptr(n_states), C, Smax, K, _hip.ptr(self.seqs), _hip.ptr(self.len_s),
                                                  self.N, self.T, _hip.ptr(self.trans), _hip.ptr(self.n_trans), self.Wmax,
                                                  _hip.ptr(seg.contiguous()), _hip.ptr(cnt_emit), _hip.ptr(cnt),
                                                  _hip.ptr(n_valid), _hip.ptr(valid), _hip.ptr(ws), ws.numel(),
                                                  _hip.stream_handle(d))
        _hip.check(rc, "dsp_dhmm_force_accumulate")
        return cnt_emit, cnt, n_valid, valid


_DHMM_FORCE_SHAPE = ("unsupported forced-alignment shape (1 <= C <= %d, 1 <= Wmax <= %d, 1 <= T <= 1024, 1 <= Smax <= %d, "
                     "1 <= K <= %d)" % (DHMM_DECODE_MAX_MODELS, DHMM_FORCE_MAX_WORDS, HMM_MAX_STATES, DHMM_MAX_SYMBOLS))


def dhmm_force_align(models, sym, lengths, transcripts, enter=None, with_seg=True, n_trans=None):
    """Forced alignment (include/dsp_audiorec.h: dsp_dhmm_force_align) of the symbol rows sym int32 [N, T]
    against the concatenation of their transcripts' word models from the ``DhmmModelSet`` (at most
    ``DHMM_DECODE_MAX_MODELS`` models, ``DHMM_FORCE_MAX_WORDS`` words a transcript).  ``transcripts``: a list of
    model-index sequences, or a padded [N, Wmax] array with ``n_trans``.  ``enter`` as ``dhmm_decode``'s.
    Returns (score float64 [N], seg int32 [N, Wmax, Smax] or None) on the device: seg[u, i, s] is the first
    frame of state s of word i (-1 behind the word's states and behind the transcript, and everywhere for an
    utterance whose score is +inf)."""
    if not 1 <= models.shape[0] <= DHMM_DECODE_MAX_MODELS:
        raise ValueError("forced alignment takes 1 .. %d word models, got %d" % (DHMM_DECODE_MAX_MODELS, models.shape[0]))
    trans, n_trans = _dhmm_transcripts(transcripts, n_trans, len(lengths))
    return DhmmForceUpdater(sym, lengths, trans, n_trans).align(models, enter, with_seg)


class VqTokenizer:
    """ONE vector-quantisation codebook shared by all sequences: the tokeniser in front of the discrete
    HMMs.  ``fit`` trains it by LBG binary splitting on all sequences together -- by definition the
    codebook ``models.VqClassifier(n_codes, n_iter, eps, normalize=False)`` gives for all-equal labels, bit
    for bit; ``transform`` is one ``dsp_vq_assign`` with members = 0 .. N-1.
    After ``fit``: codebook_ float64 [n_codes, F]."""

    def __init__(self, n_codes, n_iter=10, eps=0.01):
        from .models import VqClassifier
        VqClassifier(n_codes, n_iter, eps, normalize=False)  # its argument checks
        self.n_codes, self.n_iter, self.eps = int(n_codes), int(n_iter), float(eps)
        self._dev = None

    def fit(self, X, lengths):
        from .models import VqClassifier
        lengths = _as_host(lengths).astype(np.int32).reshape(-1)
        clf = VqClassifier(self.n_codes, self.n_iter, self.eps, normalize=False)
        self.codebook_ = clf.fit(_as_host(X, np.float64), np.zeros(len(lengths), np.int32), lengths).codebooks_[0]
        self._dev = None
        return self

    def transform(self, X, lengths):
        """sym int32 [N, T] on the device: each frame's nearest codeword (-1 behind a sequence's frames)."""
        import torch
        d = _hip.require_device()
        if self._dev is None or self._dev.device != torch.device(d):
            self._dev = _as_device(self.codebook_[None], torch.float64, d)
        N = len(lengths)
        _, code, _, _ = vq_assign(self._dev, np.array([self.n_codes], np.int32), X, lengths,
                                  groups=([0, N], np.arange(N)), check_finite=False)
        return code


class _CropFramePlan:
    """What the launch plans of the two crop-frame kernels (csrc/crop_frames.h) share: ``PitchTracker`` and
    ``LpcAnalyzer`` run after a ``FeatureExtractor`` call, on that call's device outputs, and validate
    their arguments without a device."""
    _takes = _plan = None  # "the pitch track takes", "the pitch plan": the error texts name the analysis

    def __init__(self, device, frame_length, frame_shift, **integers):
        for name, v in dict(frame_length=frame_length, frame_shift=frame_shift, **integers).items():
            if isinstance(v, bool) or int(v) != v:
                raise ValueError("%s must be an integer" % name)
        self.L, self.S = int(frame_length), int(frame_shift)
        if not 2 <= self.L <= 4096:
            raise ValueError("frame_length must be in 2 .. 4096")
        if self.S < 1:
            raise ValueError("frame_shift must be positive")
        self.device = device
        self._ws = None

    def frames(self, max_len):
        """Width of the per-frame outputs for clips of up to max_len samples (the widest crop)."""
        return 1 if max_len <= self.L else (int(max_len) - self.L + self.S - 1) // self.S + 1

    def _batch(self, pcm, extracted, offsets, max_len):
        """The batch a call was given (int16 samples: anything else is refused before a device is asked
        for) -> (pcm_flat, off, B, max_len, rows, ld), tensors on the device."""
        import torch
        if str(getattr(pcm, "dtype", "")) not in ("int16", "torch.int16"):
            raise ValueError("%s int16 samples (16-bit stereo channel sums in int32 are not supported)" % self._takes)
        if self.device is None:
            self.device = _hip.require_device()
        d = self.device
        pcm = _as_device(pcm, torch.int16, d)
        if offsets is None:
            if pcm.dim() != 2:
                raise ValueError("1-D packed pcm needs offsets")
            B, N = pcm.shape
            off = torch.arange(B + 1, dtype=torch.int64, device=d) * N
            true_max = N
        else:
            off = _as_device(offsets, torch.int64, d)
            B = off.numel() - 1
            true_max = None
        if max_len is None:
            max_len = true_max if true_max is not None else (int(torch.max(off[1:] - off[:-1]).item()) if B > 0 else 1)
        max_len = max(int(max_len), 1)
        rows = extracted["rows"]
        if rows.shape != (B, _hip.OUT_ROW_WORDS) or rows.dtype != torch.int32 or not rows.is_contiguous():
            raise ValueError("extracted['rows'] must be the [B, 19] int32 rows of the same batch")
        return pcm.reshape(-1), off, B, max_len, rows, self.frames(max_len)

    def _workspace(self, nbytes):
        """The plan's device workspace, grown to nbytes (0: the library refused the shape)."""
        import torch
        if nbytes == 0:
            raise ValueError("outside %s" % self._plan)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def plain_frames(self):
        """Frames of the last call that took a plain int64 fallback path (one host sync); the LPC lag
        sums have none, so 0 there."""
        import torch
        return int(self._ws[:4].view(torch.int32).item())


class PitchTracker(_CropFramePlan):
    """Launch plan for ``dsp_pitch_track`` (csrc/pitch.hip): the exact short-time
    autocorrelation of every crop frame, the smallest lag of its maximum inside
    [sample_rate // f0_max, sample_rate // f0_min] (clamped to [1, L - 1]), and the voicing decision and
    f0 derived from them on the device.  It runs after a ``FeatureExtractor`` call, on that call's
    device outputs.  The arguments are validated here, without a device."""
    _takes, _plan = "the pitch track takes", "the pitch plan"

    def __init__(self, frame_length, frame_shift, sample_rate, f0_min=60.0, f0_max=400.0, voicing=(3, 10),
                 device=None):
        super().__init__(device, frame_length, frame_shift, sample_rate=sample_rate)
        self.sample_rate = int(sample_rate)
        if self.sample_rate < 1:
            raise ValueError("sample_rate must be positive")
        f0_min, f0_max = float(f0_min), float(f0_max)
        if not 0.0 < f0_min <= f0_max or not np.isfinite(f0_max):
            raise ValueError("need 0 < f0_min <= f0_max")
        try:
            vnum, vden = voicing
        except (TypeError, ValueError):
            raise ValueError("voicing is a pair (vnum, vden)")
        if any(isinstance(v, bool) or int(v) != v for v in (vnum, vden)) or not 1 <= vnum <= vden <= 1024:
            raise ValueError("voicing needs integers 1 <= vnum <= vden <= 1024")
        self.vnum, self.vden = int(vnum), int(vden)
        self.lag_min = min(max(int(self.sample_rate // f0_max), 1), self.L - 1)
        self.lag_max = min(max(int(self.sample_rate // f0_min), 1), self.L - 1)

    def __call__(self, pcm, extracted, offsets=None, max_len=None):
        """pcm, offsets: what the ``FeatureExtractor`` call was given (int16); ``extracted``: the dict
        it returned.  -> dict of device tensors [B, frames(max_len)]: lag int32, peak and r0 int64,
        voiced bool, f0 float64; zeros (False) behind a clip's frames and in the rows of failed clips."""
        import torch
        pcm, off, B, max_len, rows, ld = self._batch(pcm, extracted, offsets, max_len)
        d = self.device
        lag = torch.zeros((B, ld), dtype=torch.int32, device=d)
        peak = torch.zeros((B, ld), dtype=torch.int64, device=d)
        r0 = torch.zeros((B, ld), dtype=torch.int64, device=d)
        lib = _hip.lib()
        ws = self._workspace(lib.dsp_pitch_workspace_bytes(B, max_len, self.L, self.S, self.lag_min, self.lag_max))
        rc = lib.dsp_pitch_track(_hip.ptr(pcm), _hip.ptr(off), B, max_len, self.L, self.S, self.lag_min, self.lag_max,
                                 _hip.ptr(rows[:, 15:]), _hip.ptr(rows[:, 17:]), _hip.ptr(rows[:, 18:]),
                                 _hip.OUT_ROW_WORDS, _hip.ptr(lag), _hip.ptr(peak), _hip.ptr(r0), ld, _hip.ptr(ws),
                                 ws.numel(), _hip.stream_handle(d))
        _hip.check(rc, "dsp_pitch_track")
        voiced = (peak > 0) & (self.vden * peak >= self.vnum * r0)
        rate = torch.tensor(float(self.sample_rate), dtype=torch.float64, device=d)
        f0 = torch.where(voiced, rate / lag.clamp(min=1).to(torch.float64), torch.zeros((), dtype=torch.float64, device=d))
        return dict(lag=lag, peak=peak, r0=r0, voiced=voiced, f0=f0)


def f0_statistics(f0, voiced):
    """mean, std, max, min, median of each row's f0 over its voiced frames (numpy, fp64, as
    compute_statistics does) -> [n, 5]; 0.0 for a row without a voiced frame."""
    f0, voiced = np.asarray(f0, np.float64), np.asarray(voiced, bool)
    out = np.zeros((f0.shape[0], 5))
    for i in range(f0.shape[0]):
        v = f0[i][voiced[i]]
        if v.size:
            out[i] = [np.mean(v), np.std(v), np.max(v), np.min(v), np.median(v)]
    return out


def lpc_window(window_type, L):
    """The Q15 table of ``dsp_lpc_autocorr``: floor(w * 32768 + 0.5) of ``create_window``'s fp64 window as
    int32 [L] (32768 = 1.0); None for the rectangular window (the kernel then takes the frame as it is)."""
    if window_type == "rectangular":
        return None
    return np.floor(create_window(window_type, int(L)) * 32768.0 + 0.5).astype(np.int32)


class LpcAnalyzer(_CropFramePlan):
    """Launch plan for ``dsp_lpc_autocorr`` + ``dsp_lpc_solve`` (csrc/lpc.hip): the exact
    integer autocorrelation r(0..order) of every Q15-windowed crop frame, then the Levinson-Durbin
    recursion and ``n_cep`` LPC cepstra in bit-defined fp64.  It runs after a ``FeatureExtractor`` call, on
    that call's device outputs, like ``PitchTracker``.  The arguments are validated here, without a device."""
    _takes, _plan = "the LPC analysis takes", "the LPC plan"

    def __init__(self, frame_length, frame_shift, order=12, n_cep=12, window_type='hamming', device=None):
        super().__init__(device, frame_length, frame_shift, order=order, n_cep=n_cep)
        self.p, self.Q = int(order), int(n_cep)
        if not 1 <= self.p <= min(32, self.L - 1):
            raise ValueError("order must be in 1 .. min(32, frame_length - 1)")
        if not 0 <= self.Q <= 64:
            raise ValueError("n_cep must be in 0 .. 64")
        self.window_type = window_type
        self.table = lpc_window(window_type, self.L)  # raises ValueError for an unknown window
        self._table_dev = None

    def __call__(self, pcm, extracted, offsets=None, max_len=None):
        """pcm, offsets: what the ``FeatureExtractor`` call was given (int16); ``extracted``: the dict
        it returned.  -> dict of device tensors with ld = frames(max_len): r int64 [B, ld, order + 1],
        a and k float64 [B, ld, order], err float64 and reached int32 [B, ld], cep float64 [B, ld, n_cep];
        zeros behind a clip's frames and in the rows of failed clips (the solve runs on all B ld rows,
        and a zero row solves to zeros)."""
        import torch
        pcm, off, B, max_len, rows, ld = self._batch(pcm, extracted, offsets, max_len)
        d, p, Q = self.device, self.p, self.Q
        r = torch.zeros((B, ld, p + 1), dtype=torch.int64, device=d)
        a = torch.empty((B, ld, p), dtype=torch.float64, device=d)
        k = torch.empty((B, ld, p), dtype=torch.float64, device=d)
        err = torch.empty((B, ld), dtype=torch.float64, device=d)
        reached = torch.empty((B, ld), dtype=torch.int32, device=d)
        cep = torch.empty((B, ld, Q), dtype=torch.float64, device=d)
        lib = _hip.lib()
        ws = self._workspace(lib.dsp_lpc_workspace_bytes(B, max_len, self.L, self.S, p))
        if self.table is not None and self._table_dev is None:
            self._table_dev = torch.as_tensor(self.table).to(d)
        rc = lib.dsp_lpc_autocorr(_hip.ptr(pcm), _hip.ptr(off), B, max_len, self.L, self.S, p, _hip.ptr(self._table_dev),
                                  _hip.ptr(rows[:, 15:]), _hip.ptr(rows[:, 17:]), _hip.ptr(rows[:, 18:]),
                                  _hip.OUT_ROW_WORDS, _hip.ptr(r), ld, _hip.ptr(ws), ws.numel(), _hip.stream_handle(d))
        _hip.check(rc, "dsp_lpc_autocorr")
        rc = lib.dsp_lpc_solve(_hip.ptr(r), B * ld, p, Q, _hip.ptr(a), _hip.ptr(k), _hip.ptr(err), _hip.ptr(reached),
                               _hip.ptr(cep) if Q else None, _hip.stream_handle(d))
        _hip.check(rc, "dsp_lpc_solve")
        return dict(r=r, a=a, k=k, err=err, reached=reached, cep=cep)


def lpcc_statistics(cep, lengths):
    """mean then std of each cepstrum over each clip's first ``lengths[i]`` frames (numpy, fp64) ->
    [n, 2 Q]; zeros for a clip without a frame."""
    cep, lengths = np.asarray(cep, np.float64), np.asarray(lengths).astype(np.int64).reshape(-1)
    Q = cep.shape[2]
    out = np.zeros((cep.shape[0], 2 * Q))
    for i in range(cep.shape[0]):
        v = cep[i, :max(int(lengths[i]), 0)]
        if len(v):
            out[i, :Q], out[i, Q:] = np.mean(v, axis=0), np.std(v, axis=0)
    return out


class _ModelIndex:
    """What ``SvcIndex``, ``GnbIndex`` and ``TreeIndex`` share: a fitted scikit-learn model uploaded once,
    float64 rows [Nq, D] in, class indices out, the rows the device cannot settle marked for the caller
    to answer with the model itself.  A subclass states its plan (the limits and ``_model_in_plan``),
    the fitted attribute a model's upload is recognised by (``_source``), the C entry (``_call``) with
    its leading arguments (``_args``, the model's), and a launch's rows and scratch.  One query at a
    time per index (the workspace is a launch's scratch)."""

    DMAX, CMIN, CMAX = 4096, 1, 64  # the kernels' plans: 1 <= D <= DMAX features, CMIN <= classes <= CMAX
    _counter = "uncertified"  # the stats key of a query's count

    @classmethod
    def source_of(cls, model):
        """The object a refit replaces (None before the first fit): an index is the fitted model's
        while ``index.source is source_of(model)``."""
        return getattr(model, cls._source, None)

    @classmethod
    def in_plan(cls, model, X=None):
        """model is fitted and inside the kernel's plan, and X is dense: what the constructor and
        ``query`` take.  Asks neither a device nor the library."""
        from scipy.sparse import issparse
        return not issparse(X) and cls.source_of(model) is not None and cls._model_in_plan(model)

    @classmethod
    def _shape_in_plan(cls, D, C):
        return 1 <= D <= cls.DMAX and cls.CMIN <= C <= cls.CMAX

    def __init__(self, model):
        if not self.in_plan(model):
            raise ValueError("%s outside the device plan (fitted%s, 1 <= D <= %d, %d <= classes <= %d)"
                             % (type(model).__name__, self._kind, self.DMAX, self.CMIN, self.CMAX))
        self.device = _hip.require_device()
        self.source = self.source_of(model)
        self._ws = None

    def _rows_per_launch(self, Nq):
        return Nq  # the scratch does not grow with the rows

    def _counter_offset(self, n):
        return 0  # where a launch of n rows leaves its int32 count in the workspace

    def _query(self, X, outputs, stats):
        """The outputs of a query, one per entry of ``outputs``: (dtype,) for [Nq], (dtype, w) for
        [Nq, w], None for an output not asked for.  The rows go through the C call in launches of
        ``_rows_per_launch``; a dict passed as ``stats`` receives the launches' summed count."""
        import torch
        d = self.device
        q = _as_device(X, torch.float64, d)
        if q.dim() != 2 or q.shape[1] != self.D:
            raise ValueError("X has shape %s, the model was fitted on %d features" % (tuple(q.shape), self.D))
        Nq = q.shape[0]
        outs = [None if o is None else torch.empty(Nq, *o[1:], dtype=o[0], device=d) for o in outputs]
        predict, stream = getattr(_hip.lib(), self._call), _hip.stream_handle(d)
        step, count = max(self._rows_per_launch(Nq), 1), 0
        for lo in range(0, Nq, step):
            n = min(step, Nq - lo)
            nbytes = self._workspace_bytes(n)
            if nbytes == 0:
                raise ValueError("outside the device plan")
            if self._ws is None or self._ws.numel() < nbytes:
                self._ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
            # rows [lo, lo + n) of the queries and of every output (all of them: the usual single launch)
            part = [q] + outs if n == Nq else [None if t is None else t[lo:lo + n] for t in [q] + outs]
            at = [None if t is None else t.data_ptr() for t in part]
            # after the model's own arguments the three predict calls end alike
            rc = predict(*self._args, at[0], n, *at[1:], self._ws.data_ptr(), self._ws.numel(), stream)
            _hip.check(rc, self._call)
            if stats is not None:
                off = self._counter_offset(n)
                count += int(self._ws[off:off + 4].view(torch.int32).item())
        if stats is not None:
            stats[self._counter] = count
        return outs


class SvcIndex(_ModelIndex):
    """A fitted ``sklearn.svm.SVC(kernel='rbf')`` uploaded once for ``dsp_svc_predict``
    (csrc/svm.hip): libsvm's own arrays -- support_vectors_, _n_support, _dual_coef_, _intercept_,
    _gamma (the underscore attributes: the public ones are sign-flipped for two classes).
    ``query`` is SVC.predict's vote as class indices plus, per row, whether the device could certify
    it; the caller answers uncertified rows with the model itself."""

    CMIN = 2
    WORKSPACE_CAP = 256 << 20  # a query batch is cut into launches whose scratch stays below this
    _source, _call = "support_vectors_", "dsp_svc_predict"
    _kind = " on dense rows with the rbf kernel, without probability or break_ties"

    @classmethod
    def _model_in_plan(cls, m):
        return (m.kernel == 'rbf' and not m.probability and not m.break_ties and not getattr(m, '_sparse', False)
                and cls._shape_in_plan(m.support_vectors_.shape[1], len(m.classes_)))

    def __init__(self, model):
        import torch
        super().__init__(model)
        sv = np.asarray(self.source, dtype=np.float64)
        self.nSV, self.D = sv.shape
        self.C = len(model.classes_)
        self.P = self.C * (self.C - 1) // 2
        self.gamma = float(model._gamma)
        self.sv = _as_device(sv, torch.float64, self.device)
        self.n_support = _as_device(model._n_support, torch.int32, self.device)
        self.dual_coef = _as_device(np.asarray(model._dual_coef_, dtype=np.float64).reshape(self.C - 1, self.nSV),
                                    torch.float64, self.device)
        self.intercept = _as_device(np.asarray(model._intercept_, dtype=np.float64).reshape(self.P),
                                    torch.float64, self.device)
        self._args = (*map(_hip.ptr, (self.sv, self.n_support, self.dual_coef, self.intercept)), self.nSV, self.D,
                      self.C, self.gamma)

    def _rows_per_launch(self, Nq):
        return max(1024, self.WORKSPACE_CAP // (8 * self.C * self.C))  # (C (C-1) + C) doubles per row and part

    def _workspace_bytes(self, n):
        return _hip.lib().dsp_svc_workspace_bytes(self.nSV, n, self.D, self.C)

    def _counter_offset(self, n):
        return _hip.lib().dsp_svc_workspace_uncertified_offset(self.nSV, n, self.D, self.C)

    def query(self, X, with_dec=False, stats=None):
        """(pred int32 [Nq] class index, dec float64 [Nq, C(C-1)/2] with libsvm's signs or None,
        certified int32 [Nq]); a dict passed as ``stats`` receives "uncertified" (one host sync)."""
        import torch
        dec = (torch.float64, self.P) if with_dec else None
        return tuple(self._query(X, [(torch.int32,), dec, (torch.int32,)], stats))


def gaussian_nb_fit(X, y_codes, n_classes, var_smoothing=1e-9):
    """``GaussianNB(var_smoothing=...).fit`` on the device (csrc/gnb.hip, dsp_gnb_fit): X float64
    [N, D] (D >= 2) and class codes in [0, n_classes).  Returns device tensors (theta [C, D],
    var [C, D] with epsilon added, class_count int64 [C], epsilon [1]) -- numpy's bits."""
    import torch
    d = _hip.require_device()
    X = _as_device(X, torch.float64, d)
    y = _as_device(y_codes, torch.int32, d)
    if X.dim() != 2 or y.shape != (X.shape[0],):
        raise ValueError("X must be [N, D] and y_codes [N]")
    N, D = X.shape
    C = int(n_classes)
    theta = torch.empty((C, D), dtype=torch.float64, device=d)
    var = torch.empty((C, D), dtype=torch.float64, device=d)
    count = torch.empty(C, dtype=torch.int64, device=d)
    eps = torch.empty(1, dtype=torch.float64, device=d)
    ws = torch.empty(max(D, 1) * 8, dtype=torch.uint8, device=d)
    _hip.check(_hip.lib().dsp_gnb_fit(_hip.ptr(X), _hip.ptr(y), N, D, C, float(var_smoothing), _hip.ptr(theta),
                                      _hip.ptr(var), _hip.ptr(count), _hip.ptr(eps), _hip.ptr(ws), ws.numel(),
                                      _hip.stream_handle(d)), "dsp_gnb_fit")
    return theta, var, count, eps


class GnbIndex(_ModelIndex):
    """A fitted ``sklearn.naive_bayes.GaussianNB`` uploaded once for ``dsp_gnb_predict``
    (csrc/gnb.hip): theta_, var_ and the two per-class constants of _joint_log_likelihood, computed
    here with numpy exactly as scikit-learn does.  ``query`` is GaussianNB.predict's argmax as class
    indices plus, per row, whether the device could certify it; the caller answers
    uncertified rows with the model itself."""

    WORKSPACE_CAP = 256 << 20  # a query batch is cut into launches whose scratch stays below this
    _source, _call, _kind = "theta_", "dsp_gnb_predict", ""

    @classmethod
    def _model_in_plan(cls, m):
        return cls._shape_in_plan(m.theta_.shape[1], m.theta_.shape[0])

    def __init__(self, model):
        import torch
        super().__init__(model)
        theta = np.asarray(model.theta_, dtype=np.float64)
        var = np.asarray(model.var_, dtype=np.float64)
        self.C, self.D = theta.shape
        with np.errstate(divide='ignore'):
            log_prior = np.log(np.asarray(model.class_prior_, dtype=np.float64))
        nconst = -0.5 * np.sum(np.log(2.0 * np.pi * var), axis=1)
        self.theta = _as_device(theta, torch.float64, self.device)
        self.var = _as_device(var, torch.float64, self.device)
        self.log_prior = _as_device(log_prior, torch.float64, self.device)
        self.nconst = _as_device(nconst, torch.float64, self.device)
        self._args = (*map(_hip.ptr, (self.theta, self.var, self.log_prior, self.nconst)), self.D, self.C)

    def _rows_per_launch(self, Nq):
        return max(1024, self.WORKSPACE_CAP // (16 * self.C))  # a launch's scratch: 2 C doubles per row

    def _workspace_bytes(self, n):
        return _hip.lib().dsp_gnb_workspace_bytes(n, self.D, self.C)

    def query(self, X, with_jll=False, stats=None):
        """(pred int32 [Nq] class index, jll float64 [Nq, C] or None, certified int32 [Nq]); a dict
        passed as ``stats`` receives "uncertified" (one host sync)."""
        import torch
        jll = (torch.float64, self.C) if with_jll else None
        return tuple(self._query(X, [(torch.int32,), jll, (torch.int32,)], stats))


class TreeIndex(_ModelIndex):
    """A fitted single-output ``sklearn.tree.DecisionTreeClassifier`` uploaded once for
    ``dsp_tree_predict`` (csrc/tree.hip): tree_'s children, features and thresholds and every
    node's majority class.  ``query`` is predict (as class indices) and apply; a row with a NaN
    (scikit-learn's missing value) or a value that is not finite as float32 (scikit-learn refuses
    it) comes back as -1, for the caller to hand to the model itself."""

    CMAX = (1 << 31) - 1  # a class index is an int32
    _source, _call, _kind, _counter = "tree_", "dsp_tree_predict", " with a single output", "unanswered"

    @classmethod
    def _model_in_plan(cls, m):
        return m.n_outputs_ == 1 and cls._shape_in_plan(m.n_features_in_, m.n_classes_)

    def __init__(self, model):
        import torch
        super().__init__(model)
        t = self.source
        self.n_nodes, self.max_depth, self.D = int(t.node_count), int(t.max_depth), int(model.n_features_in_)
        leaf_class = np.argmax(t.value[:, 0, :], axis=1)
        self.left = _as_device(t.children_left, torch.int32, self.device)
        self.right = _as_device(t.children_right, torch.int32, self.device)
        self.feature = _as_device(t.feature, torch.int32, self.device)
        self.threshold = _as_device(t.threshold, torch.float64, self.device)
        self.leaf_class = _as_device(leaf_class, torch.int32, self.device)
        self._args = (*map(_hip.ptr, (self.left, self.right, self.feature, self.threshold, self.leaf_class)),
                      self.n_nodes, self.max_depth, self.D)
        self._nbytes = _hip.lib().dsp_tree_workspace_bytes(self.n_nodes)

    def _workspace_bytes(self, n):
        return self._nbytes  # the packed node table, whatever the rows

    def query(self, X, with_leaf=True, stats=None):
        """(pred int32 [Nq] class index or -1, leaf int32 [Nq] node index or -1, or None); a dict
        passed as ``stats`` receives "unanswered" (one host sync)."""
        import torch
        return tuple(self._query(X, [(torch.int32,), (torch.int32,) if with_leaf else None], stats))


def zscore_fit(X):
    """normalize_features' mean/std (src/feature_extraction.py:171-177) on the device: bit for bit
    ``np.mean(X, axis=0)`` and ``np.std(X, axis=0)`` (0 -> 1) of a C-contiguous float64 [N, D] array,
    one column (numpy's pairwise order) included.  Any other layout is made C-contiguous first --
    the reference's callers build C-ordered arrays -- so a Fortran-ordered X gets the C-ordered
    array's sums, which numpy's own sums over that layout need not equal."""
    import torch
    d = _hip.require_device()
    X = _as_device(X, torch.float64, d)
    N, D = X.shape
    mean = torch.empty(D, dtype=torch.float64, device=d)
    std = torch.empty(D, dtype=torch.float64, device=d)
    _hip.check(_hip.lib().dsp_zscore_fit(_hip.ptr(X), N, D, _hip.ptr(mean), _hip.ptr(std),
                                         _hip.stream_handle(d)), "dsp_zscore_fit")
    return mean, std


def zscore_apply(X, mean, std):
    import torch
    d = _hip.require_device()
    X = _as_device(X, torch.float64, d)
    mean = _as_device(mean, torch.float64, d)
    # a private float64 copy: std may be a read-only (e.g. broadcast) numpy view
    std = _as_device(std, torch.float64, d)
    std = torch.where(std == 0, torch.ones_like(std), std)
    out = torch.empty_like(X)
    N, D = X.shape
    _hip.check(_hip.lib().dsp_zscore_apply(_hip.ptr(X), N, D, _hip.ptr(mean), _hip.ptr(std), _hip.ptr(out),
                                           _hip.stream_handle(d)), "dsp_zscore_apply")
    return out


# ---- MLP classifier (csrc/mlp.hip; models.MLPTrainer is the reference-shaped surface) ---------

def _int_array(values):
    import ctypes
    values = [int(v) for v in values]
    return (ctypes.c_int * max(len(values), 1))(*values), len(values)


def mlp_param_count(input_size, hidden_layers, num_classes):
    """Length of the packed nn.Linear parameter buffer (weight [out, in], bias [out], per layer)."""
    prev, n = int(input_size), 0
    for h in list(hidden_layers) + [num_classes]:
        n += prev * int(h) + int(h)
        prev = int(h)
    return n


def mlp_lds_bytes(input_size, hidden_layers, num_classes, batch_size):
    """dsp_mlp_lds_bytes: LDS of the fused trainer, 0 when the shape is outside its plan.  Needs the
    built library, not a GPU."""
    arr, n = _int_array(hidden_layers)
    return int(_hip.lib().dsp_mlp_lds_bytes(int(input_size), n, arr, int(num_classes), int(batch_size)))


def mlp_drop_threshold(p):
    """(drop_threshold uint32, keep_scale float32 value) of dropout probability p (include/dsp_audiorec.h)."""
    if not p:
        return 0, 1.0
    return min(int(float(p) * 4294967296.0), 4294967295), float(np.float32(1.0 / (1.0 - float(p))))


def mlp_train(X, y, hidden_layers, num_classes, perm, params, m, v, steps, lr, seeds, batch_size,
              dropout=0.3, perm_stride=0):
    """dsp_mlp_train on device tensors: X float32 [N, D], y int32 [N] (or one set per model: [n_models,
    N, D] and [n_models, N]), perm int32 [n_epochs, N] (or
    [n_models, n_epochs, N] with perm_stride = n_epochs * N), params / m / v float32 [n_models, P],
    steps int64 [n_models], lr float64 [n_models], seeds int32 [n_models] (the uint32 seeds' bit
    patterns).  Updates params, m, v, steps in place; returns (loss_hist, acc_hist) float32
    [n_models, n_epochs] on the device.  Stream-ordered, no host sync."""
    import torch
    d = X.device
    N, D = X.shape[-2:]
    n_models = params.shape[0]
    x_stride = N * D if X.dim() == 3 else 0
    y_stride = N if y.dim() == 2 else 0
    assert X.dim() == 2 or X.shape[0] == n_models
    assert y.shape[-1] == N and y.is_contiguous() and (y.dim() == 1 or y.shape[0] == n_models)
    n_epochs = perm.shape[-2]
    assert perm.shape[-1] == N and perm.dtype == torch.int32 and perm.is_contiguous()
    assert X.dtype == torch.float32 and y.dtype == torch.int32 and X.is_contiguous()
    for t in (params, m, v):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == params.shape
    assert steps.dtype == torch.int64 and lr.dtype == torch.float64 and seeds.dtype == torch.int32
    assert steps.numel() == n_models and lr.numel() == n_models and seeds.numel() == n_models
    assert params.shape[1] == mlp_param_count(D, hidden_layers, num_classes)
    loss = torch.empty((n_models, n_epochs), dtype=torch.float32, device=d)
    acc = torch.empty((n_models, n_epochs), dtype=torch.float32, device=d)
    arr, nh = _int_array(hidden_layers)
    thr, scale = mlp_drop_threshold(dropout)
    rc = _hip.lib().dsp_mlp_train(_hip.ptr(X), _hip.ptr(y), N, x_stride, y_stride, D, nh, arr, int(num_classes), n_models, n_epochs,
                                  int(batch_size), _hip.ptr(perm), int(perm_stride), _hip.ptr(params), _hip.ptr(m),
                                  _hip.ptr(v), _hip.ptr(steps), _hip.ptr(lr), _hip.ptr(seeds), thr, scale,
                                  _hip.ptr(loss), _hip.ptr(acc), _hip.stream_handle(d))
    _hip.check(rc, "dsp_mlp_train")
    return loss, acc


def mlp_predict(params, X, hidden_layers, num_classes, with_logits=False):
    """dsp_mlp_predict: (pred int32 [Nq], logits float32 [Nq, C] or None) of one packed model."""
    import torch
    d = _hip.require_device()
    X = _as_device(X, torch.float32, d)
    params = _as_device(params, torch.float32, d).reshape(-1)
    Nq, D = X.shape
    assert params.numel() == mlp_param_count(D, hidden_layers, num_classes)
    pred = torch.empty(Nq, dtype=torch.int32, device=d)
    logits = torch.empty((Nq, int(num_classes)), dtype=torch.float32, device=d) if with_logits else None
    arr, nh = _int_array(hidden_layers)
    rc = _hip.lib().dsp_mlp_predict(_hip.ptr(params), _hip.ptr(X), Nq, D, nh, arr, int(num_classes), _hip.ptr(pred),
                                    _hip.ptr(logits), _hip.stream_handle(d))
    _hip.check(rc, "dsp_mlp_predict")
    return pred, logits


def mlp_dropout_mask(seed, step, layer, rows, width, dropout=0.3):
    """dsp_mlp_dropout_mask: the trainer's keep mask uint8 [rows, width] (1 = kept)."""
    import torch
    d = _hip.require_device()
    mask = torch.empty((rows, width), dtype=torch.uint8, device=d)
    thr, _ = mlp_drop_threshold(dropout)
    rc = _hip.lib().dsp_mlp_dropout_mask(int(seed) & 0xFFFFFFFF, int(step), int(layer), int(rows), int(width), thr,
                                         _hip.ptr(mask), _hip.stream_handle(d))
    _hip.check(rc, "dsp_mlp_dropout_mask")
    return mask
