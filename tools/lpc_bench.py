#!/usr/bin/env python
"""tools/lpc_bench.py [--out profiles/lpc_bench.json] [--clips 100000] [--replays 5] [--corpus 2000]: the
exact LPC analysis (csrc/lpc.hip) at the headline shape: --clips synthetic clips of 1 s
(src.synth.make_batch_device) through the fused extraction, then dsp_lpc_autocorr (p = 12, the Q15
Hamming table) and dsp_lpc_solve (Q = 12) on its packed rows at L = 1102, S = 441.

Timed with device events, the median of --replays calls after two warm-up calls, on buffers made once,
all in one run:
  the fused extraction, dsp_pitch_track (lags 110 .. 735: the yardstick dsp_lpc_autocorr must not exceed),
    dsp_lpc_autocorr, checked against the restatement on a full-scale edge batch, and dsp_lpc_solve on all
    B ld rows;
  dsp_lpc_autocorr again on the first --loud clips amplified 8 x and clipped to int16 (recordings driven
    into full scale);
  the frames on a plain fallback path (the workspace's counter: 0 by definition);
  the restatement (tests/lpc_reference.py) on every --sample-th clip, integers and doubles checked equal;
  the 3-NN accuracy on 300 host-synthesised labelled clips (seed 7, 80 / 20 stratified, random_state 42,
    z-scored columns) for the 15-d vector, 15 + 24 cepstral statistics and the 24 statistics alone, with
    and without the window;
  with --corpus n > 0, compare(hmm=True, dtw=True) with and without lpc=6 on n labelled clips
    (src.synth.make_batch, the corpus of DESIGN.md §4.9) written as WAV files to a temporary directory."""
import argparse
import json
import os
import sys
import tempfile
import time
import wave

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dsp-audioreclabs_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dtw_bench as D  # noqa: E402

L, S, P_ORDER, Q, RATE = 1102, 441, 12, 12, 44100
LAG_MIN, LAG_MAX = 110, 735


def knn3(X, y):
    from sklearn.model_selection import train_test_split
    from src.feature_extraction import normalize_features
    from src.models import create_classifier
    tr, te, y_tr, y_te = train_test_split(X, y, test_size=0.2, random_state=42, stratify=y)
    tr, m, sd = normalize_features(tr)
    te, _, _ = normalize_features(te, m, sd)
    clf = create_classifier('knn', n_neighbors=3).fit(tr, y_tr)
    return float(np.mean(np.asarray(clf.predict(te)) == y_te))


def accuracy_rows(dev):
    from src.pipeline import FeatureExtractor, LpcAnalyzer, lpcc_statistics
    from src.synth import make_batch
    pcm, y = make_batch(300, base_seed=7, with_labels=True)
    pcm_t = torch.as_tensor(pcm).to(dev)
    out = FeatureExtractor(L, S, "hamming", True)(pcm_t)
    ok = ((out["status"] & 0xFF) == 0).cpu().numpy()
    feat = out["feat"].cpu().numpy().astype(np.float64)[ok]
    nf = out["n_frames"].cpu().numpy()[ok]
    res = dict(clips=int(ok.sum()), frames=int(nf.sum()), features_15d=knn3(feat, y[ok]))
    for window in ("hamming", "rectangular"):
        an = LpcAnalyzer(L, S, P_ORDER, Q, window)(pcm_t, out)
        stats = lpcc_statistics(an["cep"].cpu().numpy()[ok], nf)
        inside = np.arange(an["reached"].shape[1])[None, :] < nf[:, None]
        res[window] = dict(features_39d=knn3(np.concatenate([feat, stats], axis=1), y[ok]), lpcc_statistics_24d=knn3(stats, y[ok]),
                           frames_stopped_early=int((an["reached"].cpu().numpy()[ok][inside] < P_ORDER).sum()),
                           max_abs_k=float(an["k"].abs().max().item()))
    return res


def edge_batch(entry, dev):
    """A +-full-scale square wave, a DC offset of 20 000 with full-scale excursions, full-scale noise, a quiet
    clip and a constant one through ``entry`` at 1102 / 441 / 12 and 64 / 16 / 32, windowed and not, behind
    an odd lead: equal to the restatement?  And the frames counted on a plain path beside the frames with a
    sample z >= 32640 or z < -32896 (what a byte-digit form must send there)."""
    import lpc_reference as R
    import pitch_reference as P
    from src import _hip
    from src.pipeline import lpc_window
    rng = np.random.default_rng(11)
    dc = (20000 + rng.integers(-300, 300, 4002)).astype(np.int16)
    dc[[700, 1900, 3500]] = [-32768, 32767, -32768]
    clips = [np.where((np.arange(5000) // 7) % 2 == 0, 32767, -32768).astype(np.int16), dc,
             rng.integers(-32768, 32768, 5000).astype(np.int16), rng.integers(-3000, 3000, 4001).astype(np.int16),
             np.full(3000, 1234, np.int16)]
    crops = np.array([(0, 5000), (1, 4002), (3, 4999), (5, 3990), (0, 3000)], np.int32)
    lens = np.array([len(c) for c in clips])
    off = 3 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pcm = np.concatenate([np.zeros(3, np.int16)] + clips + [np.zeros(8, np.int16)])
    t = lambda a: torch.as_tensor(a).to(dev)
    pcm_t, off_t, se_t, st_t = t(pcm), t(off), t(crops), t(np.zeros(5, np.int32))
    ws = torch.zeros(256, dtype=torch.uint8, device=dev)
    equal, plain, wide = True, 0, 0
    for L_, S_, p_ in ((1102, 441, 12), (64, 16, 32)):
        nf = np.array([P.frame_count(e - s, L_, S_) for s, e in crops], np.int32)
        ld = int(nf.max())
        for window in ("rectangular", "hamming"):
            table = lpc_window(window, L_)
            table_t, nf_t = (t(table) if table is not None else None), t(nf)
            r = torch.full((5, ld, p_ + 1), -7, dtype=torch.int64, device=dev)
            _hip.check(entry(_hip.ptr(pcm_t), _hip.ptr(off_t), 5, int(lens.max()), L_, S_, p_, _hip.ptr(table_t),
                             _hip.ptr(se_t), _hip.ptr(nf_t), _hip.ptr(st_t), 0, _hip.ptr(r), ld, _hip.ptr(ws), 256,
                             _hip.stream_handle(dev)), "dsp_lpc_autocorr")
            want = R.autocorr_batch(clips, crops, nf, np.zeros(5, np.int32), L_, S_, p_, table, ld, -7)
            equal = equal and np.array_equal(r.cpu().numpy(), want)
            plain += int(ws[:4].view(torch.int32).item())
            for b, x in enumerate(clips):
                y = x.astype(np.int64) - P.centre(x)
                for f in range(nf[b]):
                    z = R.apply_window(P.frame(y, int(crops[b][0]), int(crops[b][1]), f, L_, S_), table)
                    wide += bool(((z >= 32640) | (z < -32896)).any())
    return dict(equal_restatement=bool(equal), plain_path_frames=plain, frames_with_an_unfit_digit=wide)


def corpus_rows(n):
    import compare_feature_methods as cfm
    from src.synth import make_batch
    pcm, y = make_batch(n, with_labels=True)
    with tempfile.TemporaryDirectory() as root:
        for c in sorted(set(y.tolist())):
            os.mkdir(os.path.join(root, "c%02d" % c))
        for i in range(n):
            with wave.open(os.path.join(root, "c%02d" % y[i], "s%05d.wav" % i), "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(RATE)
                w.writeframes(pcm[i].tobytes())
        return dict(clips=n, without_lpc=cfm.compare(root, hmm=True, dtw=True), lpc_6=cfm.compare(root, hmm=True, dtw=True, lpc=6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lpc_bench.json"))
    ap.add_argument("--clips", type=int, default=100000)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--sample", type=int, default=5000)
    ap.add_argument("--corpus", type=int, default=0)
    ap.add_argument("--loud", type=int, default=20000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpc_bench needs the MI355X: nothing is measured without it")
    import lpc_reference as R
    from src import _hip
    from src.pipeline import FeatureExtractor, lpc_window
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
    se, nfp, stp = _hip.ptr(rows[:, 15:]), _hip.ptr(rows[:, 17:]), _hip.ptr(rows[:, 18:])
    stream = _hip.stream_handle(dev)
    ms = dict(extraction=ms_fx)

    # the yardstick: the pitch track of the same batch
    lag = torch.zeros((B, ld), dtype=torch.int32, device=dev)
    peak = torch.zeros((B, ld), dtype=torch.int64, device=dev)
    r0 = torch.zeros((B, ld), dtype=torch.int64, device=dev)
    ws = torch.zeros(256, dtype=torch.uint8, device=dev)
    _, ms["pitch_track"] = D.timed(lambda: _hip.check(lib.dsp_pitch_track(
        _hip.ptr(pcm), _hip.ptr(off), B, N, L, S, LAG_MIN, LAG_MAX, se, nfp, stp, _hip.OUT_ROW_WORDS, _hip.ptr(lag),
        _hip.ptr(peak), _hip.ptr(r0), ld, _hip.ptr(ws), 256, stream), "dsp_pitch_track"), args.replays)
    del lag, peak, r0

    table = torch.as_tensor(lpc_window("hamming", L)).to(dev)
    r = torch.zeros((B, ld, P_ORDER + 1), dtype=torch.int64, device=dev)
    assert lib.dsp_lpc_workspace_bytes(B, N, L, S, P_ORDER) <= 256

    _, ms["lpc_autocorr"] = D.timed(lambda: _hip.check(lib.dsp_lpc_autocorr(
        _hip.ptr(pcm), _hip.ptr(off), B, N, L, S, P_ORDER, _hip.ptr(table), se, nfp, stp, _hip.OUT_ROW_WORDS, _hip.ptr(r), ld,
        _hip.ptr(ws), 256, stream), "dsp_lpc_autocorr"), args.replays)
    plain = int(ws[:4].view(torch.int32).item())

    # clipped recordings: the same crops, the samples amplified into full scale
    loud = None
    nl = min(args.loud, B)
    if nl > 0:
        keep = pcm[:nl].clone()
        pcm[:nl] = (keep.to(torch.int32) * 8).clamp(-32768, 32767).to(torch.int16)
        r2 = torch.zeros((nl, ld, P_ORDER + 1), dtype=torch.int64, device=dev)
        _, t_ms = D.timed(lambda: _hip.check(lib.dsp_lpc_autocorr(
            _hip.ptr(pcm), _hip.ptr(off), nl, N, L, S, P_ORDER, _hip.ptr(table), se, nfp, stp, _hip.OUT_ROW_WORDS,
            _hip.ptr(r2), ld, _hip.ptr(ws), 256, stream), "dsp_lpc_autocorr"), args.replays)
        loud = dict(clips=nl, ms_median=float(np.median(t_ms)), plain_path_frames=int(ws[:4].view(torch.int32).item()))
        del r2
        loud["frames"] = int(rows[:nl, 17][(rows[:nl, 18] & 0xFF) == 0].sum().item())
        pcm[:nl] = keep
        del keep

    n_rows = B * ld
    a = torch.empty((n_rows, P_ORDER), dtype=torch.float64, device=dev)
    k = torch.empty((n_rows, P_ORDER), dtype=torch.float64, device=dev)
    err = torch.empty(n_rows, dtype=torch.float64, device=dev)
    reached = torch.empty(n_rows, dtype=torch.int32, device=dev)
    cep = torch.empty((n_rows, Q), dtype=torch.float64, device=dev)
    _, ms["lpc_solve"] = D.timed(lambda: _hip.check(lib.dsp_lpc_solve(
        _hip.ptr(r), n_rows, P_ORDER, Q, _hip.ptr(a), _hip.ptr(k), _hip.ptr(err), _hip.ptr(reached), _hip.ptr(cep), stream),
        "dsp_lpc_solve"), args.replays)

    h = rows.cpu().numpy()
    ok = (h[:, 18] & 0xFF) == 0
    frames = int(h[ok, 17].sum())
    med = {name: float(np.median(v)) for name, v in ms.items()}
    res = dict(device=torch.cuda.get_device_name(0), clips=B, clip_samples=N, frame_length=L, frame_shift=S, order=P_ORDER,
               n_cep=Q, window="hamming", clips_ok=int(ok.sum()), frames=frames, solve_rows=n_rows,
               ms_median=med, ms_all={name: [float(x) for x in v] for name, v in ms.items()},
               autocorr_no_slower_than_pitch_track=bool(med["lpc_autocorr"] <= med["pitch_track"]),
               edge_batch=edge_batch(lib.dsp_lpc_autocorr, dev), clipped_batch=loud, plain_path_frames=plain,
               defined_multiply_adds=frames * sum(L - tau for tau in range(P_ORDER + 1)),
               frames_stopped_early=int((reached.view(B, ld).cpu().numpy()[ok][np.arange(ld)[None, :] < h[ok, 17][:, None]]
                                         < P_ORDER).sum()))
    sel = np.flatnonzero(ok)[::args.sample]
    clips = pcm[sel].cpu().numpy()
    t0 = time.perf_counter()
    want_r = R.autocorr_batch(list(clips), h[sel, 15:17], h[sel, 17], h[sel, 18], L, S, P_ORDER, lpc_window("hamming", L), ld, 0)
    want = R.solve(want_r, P_ORDER, Q)
    cpu_s = time.perf_counter() - t0
    view = lambda t, *tail: t.view(B, ld, *tail)[sel].cpu().numpy().reshape(len(sel) * ld, *tail)
    got = (view(a, P_ORDER), view(k, P_ORDER), view(err), view(reached), view(cep, Q))
    equal = np.array_equal(r[sel].cpu().numpy(), want_r) and np.array_equal(got[3], want[3]) and all(
        np.array_equal(g.view(np.uint64), np.ascontiguousarray(w).view(np.uint64)) for g, w in zip(got[:3] + got[4:], want[:3] + want[4:]))
    res["restatement"] = dict(sampled_clips=int(len(sel)), sample_s=cpu_s, scaled_s=cpu_s * int(ok.sum()) / max(len(sel), 1),
                              sample_equal=bool(equal))
    del pcm, r, a, k, err, reached, cep
    res["accuracy_knn3"] = accuracy_rows(dev)
    for leg in range(2 if args.corpus > 0 else 1):  # written before the long corpus leg, and again after it
        if leg:
            res["compare_corpus"] = corpus_rows(args.corpus)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
