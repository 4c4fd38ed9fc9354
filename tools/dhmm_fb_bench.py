#!/usr/bin/env python
"""tools/dhmm_fb_bench.py [--out profiles/dhmm_fb_bench.json] [--clips 10000] [--replays 5]: forward scoring and
Baum-Welch training of the discrete HMMs (csrc/dhmm_fb.hip) on tools/dhmm_bench.py's split:
--clips synthetic clips through the fused extraction, the (E, ZCR) sequences z-scored, 80 / 20 (8 000 training
sequences, 2 000 queries at the default), 10 classes, symbols of a 64-codeword tokeniser.

Everything is timed with device events, the median of --replays calls after two warm-up calls, on buffers
made once, all in this one process.  Reported:
  dsp_dhmm_forward on 320 models of 32 states x all sequences at K = 64 beside dsp_dhmm_score on the same
    symbols in the same run: slot cells/s and the ratio of the rates (6 against 4 fp64 instructions per cell);
  dsp_dhmm_expect at the fit's list (the training pairs, 10 models of 5 states) and at 64 models of 32 states x
    all sequences: slot cells/s, the A rows written and read back (16 bytes per stored slot cell) and that
    traffic as a share of the copy rate profiles/r06vp_bench.json records;
  a Baum-Welch round split into device time, copies and host rebuild, beside a Viterbi round;
  the numpy restatement (tests/dhmm_fb_reference.py) on every 100th query, checked bit-equal;
  with --corpus n > 0, the accuracy on n host-synthesised labelled clips (dhmm_bench's corpus and split) for
    the four training x scoring combinations at 16 and 64 codewords, beside vq and hmm in the same run."""
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

import dhmm_bench as DB  # noqa: E402
import dtw_bench as D  # noqa: E402
import hmm_bench as HB  # noqa: E402


def random_prob_set(C, S, K, seed):
    """DB.random_model_set's models in the probability domain (the same draws)."""
    from src.pipeline import DhmmProbSet
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.2, 0.9, (C, S))
    return DhmmProbSet.from_arrays(rng.dirichlet(np.full(K, 0.7), (C, S)), p, 1.0 - p, np.full(C, S, np.int32))


def forward_call(models, sym, lens, dev, with_labels):
    """The bare dsp_dhmm_forward call on buffers made once."""
    from src import _hip
    lib = _hip.lib()
    (N, T), (C, Smax, K) = sym.shape, models.shape
    margs = [_hip.ptr(t) for t in models.on_device(dev)] + [C, Smax, K]
    mant = torch.empty((N, C), dtype=torch.float64, device=dev)
    expo = torch.empty((N, C), dtype=torch.int32, device=dev)
    label = torch.empty(N, dtype=torch.int32, device=dev) if with_labels else None
    nbytes = lib.dsp_dhmm_fb_workspace_bytes(C, N, 0, T, Smax, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call():
        _hip.check(lib.dsp_dhmm_forward(*margs, _hip.ptr(sym), _hip.ptr(lens), N, T, _hip.ptr(mant), _hip.ptr(expo),
                                        _hip.ptr(label), _hip.ptr(ws), nbytes, _hip.stream_handle(dev)), "dsp_dhmm_forward")
        return mant, expo, label
    return call


def expect_leg(models, sym, lens, start, members, dev, replays, copy_gbs):
    """dsp_dhmm_expect through DhmmUpdater.expect (its outputs allocated per call, the workspace held)."""
    from src.pipeline import DhmmUpdater
    C, S, K = models.shape
    up = DhmmUpdater(sym, lens, start, members)
    out, ms = D.timed(lambda: up.expect(models), replays)
    plen = lens.cpu().numpy()[np.asarray(members)]
    frames = int(plen.sum())
    NS = 8 if S <= 8 else (16 if S <= 16 else 32)
    sec = HB.med(ms) * 1e-3
    # a tile (64 consecutive pairs of one group) stores and reloads S slots of all 64 lanes for every row up to
    # its longest member, not each lane's own frames
    tile_rows = sum(int(plen[p0:min(p0 + 64, start[c + 1])].max()) for c in range(C)
                    for p0 in range(int(start[c]), int(start[c + 1]), 64))
    row_bytes = tile_rows * 64 * S * 16
    return dict(pairs=len(members), models=C, n_states=S, slots=NS, K=K, ms=HB.med(ms), frames=frames,
                slot_cells_per_s=frames * NS / sec, a_row_bytes_per_stored_slot_cell=16, tile_rows=tile_rows, a_row_bytes=row_bytes,
                a_row_bytes_of_the_pairs_own_frames=frames * S * 16,
                a_row_gbs=row_bytes / sec / 1e9, a_row_share_of_copy_rate=row_bytes / sec / 1e9 / copy_gbs,
                table_bytes=len(members) * K * NS * 8, n_valid=int(out[3].sum().item()))


def corpus_accuracy(n, n_iter):
    """Accuracies on n labelled clips (DB.corpus_accuracy's corpus and split) on the (E, ZCR) sequences."""
    import compare_feature_methods as cfm
    from src.models import create_classifier
    from src.synth import make_batch
    pcm, y = make_batch(n, with_labels=True)
    with tempfile.TemporaryDirectory() as root:
        for c in sorted(set(y.tolist())):
            os.mkdir(os.path.join(root, "c%02d" % c))
        for i in range(n):
            with wave.open(os.path.join(root, "c%02d" % y[i], "s%05d.wav" % i), "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(44100)
                w.writeframes(pcm[i].tobytes())
        _, X, labels, lengths = cfm.load_both_methods(root)
    labels, lengths = np.asarray(labels), np.asarray(lengths)
    perm = np.random.default_rng(0).permutation(len(labels))
    tr, te = perm[:len(perm) * 8 // 10], perm[len(perm) * 8 // 10:]
    rows = [("dhmm_n_codes_%d_%s_%s" % (k, tn, sc), "dhmm", dict(n_codes=k, training=tn, scoring=sc, n_iter=n_iter))
            for k in (16, 64) for tn in ("viterbi", "baum_welch") for sc in ("viterbi", "forward")]
    rows += [("vq_n_codes_%d" % k, "vq", dict(n_codes=k)) for k in (16, 64)] + [("hmm", "hmm", {})]
    out = dict(clips=n, channels=int(X.shape[2]), train=len(tr), test=len(te))
    for key, kind, params in rows:
        t0 = time.perf_counter()
        clf = create_classifier(kind, **params).fit(X[tr], labels[tr], lengths=lengths[tr])
        fit_s = time.perf_counter() - t0
        pred = clf.predict(X[te], lengths=lengths[te])
        out[key] = dict(accuracy=float(np.mean(pred == labels[te])), fit_wall_s=fit_s, rounds=int(getattr(clf, "n_iter_", 0)))
        if kind == "dhmm":
            out[key]["train_accuracy"] = float(np.mean(clf.predict(X[tr], lengths=lengths[tr]) == labels[tr]))
            out[key]["last_total"] = float(clf.totals_[-1].sum()) if len(clf.totals_) else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dhmm_fb_bench.json"))
    ap.add_argument("--clips", type=int, default=10000)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--sample", type=int, default=100)
    ap.add_argument("--n-iter", type=int, default=10)
    ap.add_argument("--corpus", type=int, default=2000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dhmm_fb_bench needs the MI355X: nothing is measured without it")
    import dhmm_fb_reference as R
    from src.pipeline import (DhmmModelSet, DhmmProbSet, DhmmUpdater, VqTokenizer, dhmm_nll, hmm_uniform_segmentation)
    with open(os.path.join(REPO, "profiles", "r06vp_bench.json")) as f:
        copy_gbs = float(json.load(f)["roofline"]["measured_copy_gbs"])
    dev = torch.device("cuda", 0)
    x, lens, cut = D.sequences(args.clips, dev)
    C, S, K = 10, 5, 64
    res = dict(device=torch.cuda.get_device_name(0), clips=int(x.shape[0]), T=int(x.shape[1]), classes=C, K=K,
               isa_fp64_per_cell=dict(forward=6, viterbi=4), copy_rate_gbs_r06vp=copy_gbs,
               fp64_vector_peak_datasheet=D.FP64_VECTOR_PEAK)
    lens_h = lens.cpu().numpy()
    ref, lr, lr_h = x[:cut].contiguous(), lens[:cut].contiguous(), lens_h[:cut]
    frames_all = int(lens.sum().item())
    tok = VqTokenizer(K, args.n_iter).fit(ref, lr_h)
    sym = tok.transform(x, lens_h)

    # ---- dsp_dhmm_forward at the machine-filling shape, beside dsp_dhmm_score in the same run ----
    _, ms_v = D.timed(DB.score_call(DB.random_model_set(320, 32, K, seed=2), sym, lens, dev, False), args.replays)
    _, ms_f = D.timed(forward_call(random_prob_set(320, 32, K, seed=2), sym, lens, dev, False), args.replays)
    _, ms_fl = D.timed(forward_call(random_prob_set(320, 32, K, seed=2), sym, lens, dev, True), args.replays)
    cells = frames_all * 32 * 320
    res["forward_full"] = dict(N=int(x.shape[0]), models=320, n_states=32, forward_ms=HB.med(ms_f), forward_with_label_ms=HB.med(ms_fl),
                               viterbi_ms=HB.med(ms_v), forward_slot_cells_per_s=cells / (HB.med(ms_f) * 1e-3),
                               viterbi_slot_cells_per_s=cells / (HB.med(ms_v) * 1e-3), ratio_to_viterbi_rate=HB.med(ms_v) / HB.med(ms_f),
                               forward_share_of_no_fma_issue_rate=cells / (HB.med(ms_f) * 1e-3) * 6 / (D.FP64_VECTOR_PEAK / 2))

    # ---- dsp_dhmm_expect: the fit's list, and 64 models of 32 states x all sequences ----
    codes = (torch.arange(cut) % C).numpy()
    order = np.argsort(codes, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=C))])
    sym_tr = sym[:cut].contiguous()
    res["expect_fit_list"] = expect_leg(random_prob_set(C, S, K, seed=3), sym_tr, lr, start, order, dev, args.replays, copy_gbs)
    N = int(x.shape[0])
    big = (np.arange(N) % 64)
    order_b = np.argsort(big, kind="stable")
    start_b = np.concatenate([[0], np.cumsum(np.bincount(big, minlength=64))])
    res["expect_64x32"] = expect_leg(random_prob_set(64, 32, K, seed=4), sym, lens, start_b, order_b, dev, args.replays, copy_gbs)

    # ---- a Baum-Welch round beside a Viterbi round, phase by phase ----
    states = np.full(C, S, np.int32)
    up = DhmmUpdater(sym_tr, lr, start, order)
    seg0 = hmm_uniform_segmentation(lr_h[order], states[codes[order]], S)

    def rounds(kind, record):
        st = up.accumulate(states, K, seg0, np.zeros(len(order)))
        model = DhmmProbSet(st[0], st[2], states) if kind == "baum_welch" else DhmmModelSet(*st[:3], states)
        for _ in range(args.n_iter):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "baum_welch":
                out = up.expect(model)
            else:
                score, seg = up.align(model)
                out = up.accumulate(states, K, seg, score)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            host = [t.cpu().numpy() for t in out]
            t2 = time.perf_counter()
            if kind == "baum_welch":
                total = float(np.where(host[0] > 0, dhmm_nll(host[0], host[1]), 0.0).sum())
                model = DhmmProbSet(host[2], host[3], states, prev=model)
            else:
                total = float(host[3].sum())
                model = DhmmModelSet(*host[:3], states, prev=model)
            t3 = time.perf_counter()
            if record is not None:
                record["device_ms"].append((t1 - t0) * 1e3)
                record["copy_ms"].append((t2 - t1) * 1e3)
                record["host_ms"].append((t3 - t2) * 1e3)
                record["totals"].append(total)
        return model

    for kind in ("baum_welch", "viterbi"):
        rec = dict(device_ms=[], copy_ms=[], host_ms=[], totals=[])
        rounds(kind, None)
        model = rounds(kind, rec)
        rec.update(rounds=args.n_iter, pairs=len(order), n_states=S, K=K, device_ms_median=HB.med(rec["device_ms"]),
                   copy_ms_median=HB.med(rec["copy_ms"]), host_ms_median=HB.med(rec["host_ms"]))
        res["round_" + kind] = rec
        if kind == "baum_welch":
            prob_fit = model

    # ---- the numpy restatement on every `sample`-th query ----
    qs, lq = sym[cut:].contiguous(), lens[cut:].contiguous()
    (mant, expo, label), ms_p = D.timed(forward_call(prob_fit, qs, lq, dev, True), args.replays)
    sel = np.arange(0, qs.shape[0], args.sample)
    t0 = time.perf_counter()
    want = R.forward(R.Prob(prob_fit.pemit, prob_fit.pstay, prob_fit.padv, prob_fit.n_states), qs.cpu().numpy()[sel], lens_h[cut:][sel])
    cpu_s = time.perf_counter() - t0
    res["predict"] = dict(Nq=int(qs.shape[0]), models=C, n_states=S, forward_with_label_ms=HB.med(ms_p))
    res["numpy_restatement"] = dict(sampled_queries=int(len(sel)), sample_s=cpu_s,
                                    sample_bits_equal=bool(
                                        np.array_equal(mant.cpu().numpy()[sel].view(np.uint64), want[0].view(np.uint64))
                                        and np.array_equal(expo.cpu().numpy()[sel], want[1])
                                        and np.array_equal(label.cpu().numpy()[sel], want[2])))
    if args.corpus > 0:
        res["accuracy"] = corpus_accuracy(args.corpus, args.n_iter)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
