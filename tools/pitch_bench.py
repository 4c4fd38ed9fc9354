#!/usr/bin/env python
"""tools/pitch_bench.py [--out profiles/pitch_bench.json] [--clips 100000] [--replays 5]: the exact
autocorrelation pitch track (csrc/pitch.hip) at the headline shape: --clips synthetic
clips of 1 s (src.synth.make_batch_device) through the fused extraction, then dsp_pitch_track on its
packed rows at L = 1102, S = 441, lags 110 .. 735.

Timed with device events, the median of --replays calls after two warm-up calls, on buffers made once.
Reported:
  the kernel time, beside the fused extraction's on the same batch;
  the multiply-adds of the definition (per frame and lag the L - tau products of the sum, zero-padded
    ones included) per second, the i8 multiply-adds the kernel issues (16 x 16 x 64 per MFMA, four MFMAs
    per kept step and lag tile, counted on the host from the crops) per second, and the latter over the
    i8 matrix-core peak (256 CUs x 4 SIMDs x 1024 multiply-adds per clock at 2.4 GHz);
  the frames that took the plain int64 path;
  the numpy restatement (tests/pitch_reference.py) on every --sample-th clip, checked equal;
  the 3-NN accuracy on 300 host-synthesised labelled clips (seed 7, 80 / 20 stratified, random_state 42,
    z-scored columns) for the 15-d vector, the 20-d vector and the five f0 statistics alone."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dsp-audioreclabs_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dtw_bench as D  # noqa: E402

L, S, LAG_MIN, LAG_MAX, RATE = 1102, 441, 110, 735, 44100
I8_PEAK = 256 * 4 * 1024 * 2.4e9  # multiply-adds per second


def issued_steps(n):
    """Kept (step, tile) pairs of a frame with n valid samples: steps i0 = 0, 64, ... while
    i0 + base < n for each 256-lag tile from base = 96 (csrc/pitch.hip)."""
    tau0 = LAG_MIN & ~15
    bases = tau0 + 256 * np.arange((LAG_MAX - tau0) // 256 + 1)
    return sum(np.maximum(0, -(-(n - b) // 64)) for b in bases)


def accuracy_rows(dev):
    from sklearn.model_selection import train_test_split
    from src.feature_extraction import normalize_features
    from src.models import create_classifier
    from src.pipeline import FeatureExtractor, PitchTracker, f0_statistics
    from src.synth import make_batch
    pcm, y = make_batch(300, base_seed=7, with_labels=True)
    pcm_t = torch.as_tensor(pcm).to(dev)
    out = FeatureExtractor(L, S, "hamming", True)(pcm_t)
    track = PitchTracker(L, S, RATE)(pcm_t, out)
    ok = ((out["status"] & 0xFF) == 0).cpu().numpy()
    feat = out["feat"].cpu().numpy().astype(np.float64)[ok]
    voiced = track["voiced"].cpu().numpy()[ok]
    stats = f0_statistics(track["f0"].cpu().numpy()[ok], voiced)
    inside = np.arange(voiced.shape[1])[None, :] < out["n_frames"].cpu().numpy()[ok][:, None]
    res = dict(clips=int(ok.sum()), frames=int(inside.sum()), unvoiced_frames=int((inside & ~voiced).sum()))
    for name, X in (("features_15d", feat), ("features_20d", np.concatenate([feat, stats], axis=1)), ("f0_statistics_5d", stats)):
        tr, te, y_tr, y_te = train_test_split(X, y[ok], test_size=0.2, random_state=42, stratify=y[ok])
        tr, m, sd = normalize_features(tr)
        te, _, _ = normalize_features(te, m, sd)
        clf = create_classifier('knn', n_neighbors=3).fit(tr, y_tr)
        res[name] = float(np.mean(np.asarray(clf.predict(te)) == y_te))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pitch_bench.json"))
    ap.add_argument("--clips", type=int, default=100000)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--sample", type=int, default=5000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pitch_bench needs the MI355X: nothing is measured without it")
    import pitch_reference as P
    from src import _hip
    from src.pipeline import FeatureExtractor
    from src.synth import make_batch_device
    dev = torch.device("cuda", 0)
    lib = _hip.lib()
    B, N = args.clips, RATE
    pcm = torch.empty((B, N), dtype=torch.int16, device=dev)
    for lo in range(0, B, 2048):
        n = min(2048, B - lo)
        pcm[lo:lo + n] = make_batch_device(n, dev, start=lo)
    off = torch.arange(B + 1, dtype=torch.int64, device=dev) * N
    fx = FeatureExtractor(L, S, "hamming", True)
    out, ms_fx = D.timed(lambda: fx(pcm), args.replays)
    rows = out["rows"].clone()
    ld = (N - L + S - 1) // S + 1
    lag = torch.zeros((B, ld), dtype=torch.int32, device=dev)
    peak = torch.zeros((B, ld), dtype=torch.int64, device=dev)
    r0 = torch.zeros((B, ld), dtype=torch.int64, device=dev)
    nbytes = lib.dsp_pitch_workspace_bytes(B, N, L, S, LAG_MIN, LAG_MAX)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    def call():
        _hip.check(lib.dsp_pitch_track(_hip.ptr(pcm), _hip.ptr(off), B, N, L, S, LAG_MIN, LAG_MAX, _hip.ptr(rows[:, 15:]),
                                       _hip.ptr(rows[:, 17:]), _hip.ptr(rows[:, 18:]), _hip.OUT_ROW_WORDS, _hip.ptr(lag),
                                       _hip.ptr(peak), _hip.ptr(r0), ld, _hip.ptr(ws), nbytes, _hip.stream_handle(dev)),
                   "dsp_pitch_track")

    _, ms = D.timed(call, args.replays)
    t = float(np.median(ms)) * 1e-3
    h = rows.cpu().numpy()
    ok = (h[:, 18] & 0xFF) == 0
    nf = h[ok, 17].astype(np.int64)
    last = (h[ok, 16] - h[ok, 15]).astype(np.int64) - (nf - 1) * S  # valid samples of the last frame
    frames = int(nf.sum())
    per_frame = sum(L - tau for tau in range(LAG_MIN, LAG_MAX + 1))
    steps = int((nf - 1).sum()) * int(issued_steps(np.int64(L))) + int(issued_steps(np.minimum(last, L)).sum())
    issued = steps * 4 * 16 * 16 * 64
    res = dict(device=torch.cuda.get_device_name(0), clips=B, clip_samples=N, frame_length=L, frame_shift=S,
               lag_min=LAG_MIN, lag_max=LAG_MAX, clips_ok=int(ok.sum()), frames=frames, frames_per_clip=frames / max(int(ok.sum()), 1),
               kernel_ms=dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms))),
               extraction_ms_median=float(np.median(ms_fx)),
               plain_path_frames=int(ws[:4].view(torch.int32).item()),
               defined_multiply_adds=frames * per_frame, defined_multiply_adds_per_s=frames * per_frame / t,
               issued_i8_multiply_adds=issued, issued_i8_multiply_adds_per_s=issued / t,
               i8_peak_multiply_adds_per_s=I8_PEAK, issued_over_i8_peak=issued / t / I8_PEAK,
               mfma_per_frame=4 * int(issued_steps(np.int64(L))))
    sel = np.flatnonzero(ok)[::args.sample]
    clips = pcm[sel].cpu().numpy()
    t0 = time.perf_counter()
    want = P.track_batch(list(clips), h[sel, 15:17], h[sel, 17], h[sel, 18], L, S, LAG_MIN, LAG_MAX, ld, (0, 0, 0))
    cpu_s = time.perf_counter() - t0
    got = [v[sel].cpu().numpy() for v in (lag, peak, r0)]
    res["numpy_restatement"] = dict(sampled_clips=int(len(sel)), sample_s=cpu_s, scaled_s=cpu_s * int(ok.sum()) / max(len(sel), 1),
                                    sample_equal=bool(all(np.array_equal(g, w) for g, w in zip(got, want))))
    del pcm, lag, peak, r0
    res["accuracy_knn3"] = accuracy_rows(dev)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
