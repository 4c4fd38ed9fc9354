#!/usr/bin/env python
"""tools/dtw_bench.py [--out profiles/dtw_bench.json] [--clips 10000] [--replays 5]: the DTW
nearest-neighbour query (csrc/dtw.hip through src.pipeline.DtwIndex) at the size the classifier is
for.

Workload: --clips synthetic clips (src.synth.make_batch_device) through the fused extraction with
return_sequences, the (E, ZCR) sequences z-scored per channel over the training frames, split 80 / 20
(8 000 references, 2 000 queries at the default), k = 3, unconstrained and with window = 10.

Per leg: ``DtwIndex.query`` on sequences already on the device, timed with device events over
--replays calls after two warm-up calls (median, min and max in ms); the admissible DP cells of the
leg counted from the lengths; cells/s; fp64 operations/s at 3F + 3 per admissible cell (the counting
convention: F subtracts, F multiplies, F adds, the three-operand min as three; the kernel issues
3F + 2 instructions, and the sqrt per pair is left out); and that rate over the part's
data-sheet fp64 vector rate (78.6 TFLOP/s counts an FMA as two; the DP has no FMA -- contraction
would change the bits -- so its ceiling is half of it, reported as well).

Baseline: the vectorised numpy restatement of tests/dtw_reference.py on a 1/100 sample of the pairs
(every 100th query against all references) on this host, scaled by 100.  It is the only other
implementation of this distance that exists here (no dtaidistance, no tslearn); it is a reference
written for clarity, not a tuned CPU DTW.  The sampled queries' neighbours and distances are also
compared with the device's, bit for bit.  Prints one JSON document and writes it to --out."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dsp-audioreclabs_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12  # MI355X data sheet, vector FP64 FLOP/s with an FMA as two (not measured here)
K = 3


def sequences(n_clips, dev):
    """(padded float64 [N, T, 2] z-scored (E, ZCR) sequences, lengths int32 [N]) on the device."""
    from src.pipeline import FeatureExtractor
    from src.synth import make_batch_device
    fx = FeatureExtractor(1102, 441, "hamming", True, return_sequences=True)
    seqs, lens = [], []
    for lo in range(0, n_clips, 2048):  # chunks of make_batch_device's own size: 180 MB of PCM at a time
        n = min(2048, n_clips - lo)
        out = fx(make_batch_device(n, dev, start=lo))
        ok = (out["status"] & 0xFF) == 0
        seqs.append(out["seq"][ok][:, :, [0, 2]].to(torch.float64))
        lens.append(out["n_frames"][ok].clone())
    lens = torch.cat(lens)
    T = int(lens.max().item())
    x = torch.cat([s[:, :T] if s.shape[1] >= T else torch.nn.functional.pad(s, (0, 0, 0, T - s.shape[1]))
                   for s in seqs])
    cut = x.shape[0] * 8 // 10
    valid = torch.arange(T, device=dev)[None, :] < lens[:, None]
    frames = x[:cut][valid[:cut]]
    mean, std = frames.mean(dim=0), frames.std(dim=0, unbiased=False)
    std = torch.where(std == 0, torch.ones_like(std), std)
    x = torch.where(valid[:, :, None], (x - mean) / std, torch.zeros_like(x))
    return x.contiguous(), lens.to(torch.int32).contiguous(), cut


def admissible_cells(lq, lr, window):
    """Admissible DP cells over all (query, reference) pairs, from the two length histograms."""
    nq, cq = np.unique(lq, return_counts=True)
    nr, cr = np.unique(lr, return_counts=True)
    total = 0
    for n, a in zip(nq.tolist(), cq.tolist()):
        for m, b in zip(nr.tolist(), cr.tolist()):
            if window < 0:
                cells = n * m
            else:
                w = max(window, abs(n - m))
                i = np.arange(n)
                cells = int((np.minimum(m - 1, i + w) - np.maximum(0, i - w) + 1).clip(min=0).sum())
            total += cells * a * b
    return total


def leg(x, lens, cut, window, replays, sample):
    import dtw_reference as R
    from src.pipeline import DtwIndex
    F = x.shape[2]
    ref, lr, qs, lq = x[:cut], lens[:cut], x[cut:], lens[cut:]
    labels = torch.arange(cut, device=x.device, dtype=torch.int32) % 10
    index = DtwIndex(ref, lr, labels, K, n_classes=10, window=window, check_finite=False)
    for _ in range(2):
        out = index.query(qs, lq, check_finite=False)
    torch.cuda.synchronize()
    ms = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = index.query(qs, lq, check_finite=False)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    w = -1 if window is None else window
    cells = admissible_cells(lq.cpu().numpy(), lr.cpu().numpy(), w)
    med = float(np.median(ms))
    ops = cells * (3 * F + 3)
    r = dict(window=window, Nq=int(qs.shape[0]), Nr=int(cut), T=int(x.shape[1]), F=F, k=K,
             mean_len=float(lens.float().mean().item()), max_len=int(lens.max().item()),
             ms_median=med, ms_min=float(min(ms)), ms_max=float(max(ms)), replays=replays,
             admissible_cells=cells, cells_per_s=cells / (med * 1e-3), fp64_ops_per_cell=3 * F + 3,
             fp64_ops_per_s=ops / (med * 1e-3),
             share_of_datasheet_fp64_vector=ops / (med * 1e-3) / FP64_VECTOR_PEAK,
             share_of_no_fma_issue_rate=ops / (med * 1e-3) / (FP64_VECTOR_PEAK / 2))
    # baseline: the numpy restatement on every `sample`-th query against all references, scaled
    sel = np.arange(0, qs.shape[0], sample)
    qa, la = qs[sel].cpu().numpy(), lq[sel].cpu().numpy()
    rb, lb = ref.cpu().numpy(), lr.cpu().numpy()
    t0 = time.perf_counter()
    d = R.dtw_pairwise(qa, la, rb, lb, w)
    cpu_s = time.perf_counter() - t0
    want = R.knn_from_dist(d, K, labels.cpu().numpy())
    got = [t.cpu().numpy()[sel] for t in out]
    r.update(baseline="numpy restatement (tests/dtw_reference.py dtw_pairwise): the only other implementation here",
             baseline_sampled_queries=int(len(sel)), baseline_sample_s=cpu_s,
             baseline_scaled_s=cpu_s * qs.shape[0] / len(sel),
             speedup_over_baseline=cpu_s * qs.shape[0] / len(sel) / (med * 1e-3),
             sample_bits_equal=bool(np.array_equal(got[0], want[0]) and
                                    np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)) and
                                    np.array_equal(got[2], want[2])))
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dtw_bench.json"))
    ap.add_argument("--clips", type=int, default=10000)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--sample", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dtw_bench needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda", 0)
    x, lens, cut = sequences(args.clips, dev)
    res = dict(device=torch.cuda.get_device_name(0), clips=int(x.shape[0]), fp64_vector_peak_datasheet=FP64_VECTOR_PEAK,
               legs=[leg(x, lens, cut, w, args.replays, args.sample) for w in (None, 10)])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
