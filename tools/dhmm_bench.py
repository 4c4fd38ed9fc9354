#!/usr/bin/env python
"""tools/dhmm_bench.py [--out profiles/dhmm_bench.json] [--clips 10000] [--replays 5]: the discrete-observation
HMMs over a shared VQ codebook (csrc/dhmm.hip) at the size of tools/dtw_bench.py's split:
--clips synthetic clips through the fused extraction, the (E, ZCR) sequences z-scored, 80 / 20 (8 000 training
sequences, 2 000 queries at the default), 10 classes (the pseudo labels clip index mod 10).

Everything is timed with device events, the median of --replays calls after two warm-up calls, on buffers
made once, all in this one process.  Reported:
  dsp_hmm_score at F = 2 on 320 models of 32 states x all sequences (tools/hmm_bench.py's call): the
    yardstick, hmm_dp<2>'s slot-cell rate of this run;
  dsp_dhmm_score on 320 models of 32 states x all sequences at K = 64 and K = 256, on symbols from a 64- and
    a 256-codeword tokeniser fitted on the training part: slot cells/s and the ratio to the yardstick;
  the classifier's shape, 10 models x 5 states, K = 64, the 2 000 queries: tokenisation and score timed
    separately and together;
  the fit: one round phase by phase (align + accumulate / copies / host rebuild) and whole, and
    DiscreteHmmClassifier.fit's wall time with the tokeniser's training;
  the numpy restatement (tests/dhmm_reference.py) on every 100th query, checked bit-equal;
  with --corpus n > 0, the accuracy on n host-synthesised labelled clips, vq_bench's split, for n_codes 16
    and 64 on (E, ZCR) and on (E, ZCR, 6 LPC cepstra)."""
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
import hmm_bench as HB  # noqa: E402


def random_model_set(C, S, K, seed):
    from src.pipeline import DhmmModelSet
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.2, 0.9, (C, S))
    return DhmmModelSet.from_arrays(-np.log(rng.dirichlet(np.full(K, 0.7), (C, S))), -np.log(p), -np.log(1.0 - p),
                                    np.full(C, S, np.int32))


def score_call(models, sym, lens, dev, with_labels):
    """The bare dsp_dhmm_score call on buffers made once."""
    from src import _hip
    lib = _hip.lib()
    (N, T), (C, Smax, K) = sym.shape, models.shape
    margs = [_hip.ptr(t) for t in models.on_device(dev)] + [C, Smax, K]
    score = torch.empty((N, C), dtype=torch.float64, device=dev)
    label = torch.empty(N, dtype=torch.int32, device=dev) if with_labels else None
    nbytes = lib.dsp_dhmm_workspace_bytes(C, N, 0, T, Smax, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call():
        _hip.check(lib.dsp_dhmm_score(*margs, _hip.ptr(sym), _hip.ptr(lens), N, T, _hip.ptr(score), _hip.ptr(label),
                                      _hip.ptr(ws), nbytes, _hip.stream_handle(dev)), "dsp_dhmm_score")
        return score, label
    return call


def corpus_accuracy(n):
    """Accuracies on n labelled clips written as a WAV tree and read back by compare_feature_methods' loader,
    tools/vq_bench.py's corpus and split: the (E, ZCR) sequences and the same with 6 LPC cepstra."""
    import compare_feature_methods as cfm
    from src.models import create_classifier
    from src.synth import make_batch
    pcm, y = make_batch(n, with_labels=True)
    out = dict(clips=n)
    with tempfile.TemporaryDirectory() as root:
        for c in sorted(set(y.tolist())):
            os.mkdir(os.path.join(root, "c%02d" % c))
        for i in range(n):
            with wave.open(os.path.join(root, "c%02d" % y[i], "s%05d.wav" % i), "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(44100)
                w.writeframes(pcm[i].tobytes())
        for name, lpc in (("e_zcr", 0), ("e_zcr_lpcc6", 6)):
            _, X, labels, lengths = cfm.load_both_methods(root, lpc=lpc)
            labels, lengths = np.asarray(labels), np.asarray(lengths)
            perm = np.random.default_rng(0).permutation(len(labels))
            tr, te = perm[:len(perm) * 8 // 10], perm[len(perm) * 8 // 10:]
            rows = [("dhmm_n_codes_%d" % k, "dhmm", dict(n_codes=k)) for k in (16, 64)]
            rows += [("vq_n_codes_%d" % k, "vq", dict(n_codes=k)) for k in (16, 64)] + [("hmm", "hmm", {})]
            leg = dict(channels=int(X.shape[2]), train=len(tr), test=len(te))
            for key, kind, params in rows:
                t0 = time.perf_counter()
                clf = create_classifier(kind, **params).fit(X[tr], labels[tr], lengths=lengths[tr])
                fit_s = time.perf_counter() - t0
                pred = clf.predict(X[te], lengths=lengths[te])
                leg[key] = dict(accuracy=float(np.mean(pred == labels[te])), fit_wall_s=fit_s,
                                rounds=int(getattr(clf, "n_iter_", 0)))
            out[name] = leg
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dhmm_bench.json"))
    ap.add_argument("--clips", type=int, default=10000)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--sample", type=int, default=100)
    ap.add_argument("--n-iter", type=int, default=10)
    ap.add_argument("--corpus", type=int, default=2000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dhmm_bench needs the MI355X: nothing is measured without it")
    import dhmm_reference as R
    from src.models import DiscreteHmmClassifier
    from src.pipeline import DhmmModelSet, DhmmUpdater, VqTokenizer, hmm_uniform_segmentation
    dev = torch.device("cuda", 0)
    x, lens, cut = D.sequences(args.clips, dev)
    F, C, S = x.shape[2], 10, 5
    res = dict(device=torch.cuda.get_device_name(0), clips=int(x.shape[0]), F=F, T=int(x.shape[1]), classes=C,
               isa_fp64_per_cell=dict(dhmm=4, hmm=4 * F + 4), fp64_vector_peak_datasheet=D.FP64_VECTOR_PEAK)
    ref, lr, qs, lq = x[:cut].contiguous(), lens[:cut].contiguous(), x[cut:].contiguous(), lens[cut:].contiguous()
    frames_all, frames_q = int(lens.sum().item()), int(lq.sum().item())
    lens_h, lr_h, lq_h = lens.cpu().numpy(), lr.cpu().numpy(), lq.cpu().numpy()

    # ---- the yardstick of this run: hmm_dp<2> at the shape that fills the machine ----
    _, ms_h = D.timed(HB.score_call(HB.random_model_set(320, 32, F, seed=1), x, lens, dev, False), args.replays)
    slot_h = frames_all * 32 * 320 / (HB.med(ms_h) * 1e-3)
    res["hmm_yardstick"] = dict(score_full_ms=HB.med(ms_h), slot_cells_per_s=slot_h,
                                share_of_no_fma_issue_rate=slot_h * (4 * F + 4) / (D.FP64_VECTOR_PEAK / 2))

    # ---- dsp_dhmm_score at the same shape, K = 64 and K = 256 ----
    toks, syms = {}, {}
    for K in (64, 256):
        t0 = time.perf_counter()
        toks[K] = VqTokenizer(K, args.n_iter).fit(ref, lr_h)
        fit_s = time.perf_counter() - t0
        syms[K] = toks[K].transform(x, lens_h)
        _, ms_d = D.timed(score_call(random_model_set(320, 32, K, seed=2), syms[K], lens, dev, False), args.replays)
        slot = frames_all * 32 * 320 / (HB.med(ms_d) * 1e-3)
        res["score_full_K%d" % K] = dict(N=int(x.shape[0]), models=320, n_states=32, tokenizer_fit_wall_s=fit_s,
                                         ms=HB.med(ms_d), slot_cells_per_s=slot, ratio_to_hmm_dp2=slot / slot_h,
                                         share_of_no_fma_issue_rate=slot * 4 / (D.FP64_VECTOR_PEAK / 2))

    # ---- the classifier's shape: 10 models x 5 states, K = 64, the queries ----
    K = 64
    small = random_model_set(C, S, K, seed=3)
    sym_q = toks[K].transform(qs, lq_h)
    call_q = score_call(small, sym_q, lq, dev, True)
    _, ms_tok = D.timed(lambda: toks[K].transform(qs, lq_h), args.replays)
    _, ms_sc = D.timed(call_q, args.replays)
    _, ms_both = D.timed(lambda: (toks[K].transform(qs, lq_h), call_q()), args.replays)
    _, ms_hp = D.timed(HB.score_call(HB.random_model_set(C, S, F, seed=4), qs, lq, dev, True), args.replays)
    res["predict"] = dict(Nq=int(qs.shape[0]), models=C, n_states=S, K=K, tokenise_ms=HB.med(ms_tok), score_ms=HB.med(ms_sc),
                          tokenise_and_score_ms=HB.med(ms_both), hmm_predict_ms=HB.med(ms_hp),
                          slot_cells_per_s=frames_q * 8 * C / (HB.med(ms_sc) * 1e-3),
                          note="tokenise: VqTokenizer.transform, the call with its list upload and output allocations")

    # ---- the fit, phase by phase (DiscreteHmmClassifier.fit's loop on symbols already on the device) ----
    codes = (torch.arange(cut) % C).numpy()
    order = np.argsort(codes, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=C))])
    states = np.full(C, S, np.int32)
    up = DhmmUpdater(syms[K][:cut].contiguous(), lr, start, order)
    fit = dict(device_ms=[], copy_ms=[], host_ms=[], totals=[])

    def run_fit(record):
        seg = hmm_uniform_segmentation(lr_h[order], states[codes[order]], S)
        st = up.accumulate(states, K, seg, np.zeros(len(order)))
        model = DhmmModelSet(*st[:3], states)
        for _ in range(args.n_iter):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            score, new_seg = up.align(model)
            st = up.accumulate(states, K, new_seg, score)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            host = [t.cpu().numpy() for t in st] + [new_seg.cpu().numpy()]
            t2 = time.perf_counter()
            model = DhmmModelSet(*host[:3], states, prev=model)
            same = np.array_equal(host[4], seg)
            seg = host[4]
            t3 = time.perf_counter()
            if record:
                fit["device_ms"].append((t1 - t0) * 1e3)
                fit["copy_ms"].append((t2 - t1) * 1e3)
                fit["host_ms"].append((t3 - t2) * 1e3)
                fit["totals"].append(float(host[3].sum()))
            if same:
                break
        return model

    run_fit(False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model_fit = run_fit(True)
    torch.cuda.synchronize()
    fit.update(wall_ms=(time.perf_counter() - t0) * 1e3, rounds=len(fit["device_ms"]), pairs=len(order), n_states=S, K=K,
               device_ms_median=HB.med(fit["device_ms"]), copy_ms_median=HB.med(fit["copy_ms"]),
               host_ms_median=HB.med(fit["host_ms"]))
    (sc_f, seg_f), ms_al = D.timed(lambda: up.align(model_fit), args.replays)
    _, ms_al0 = D.timed(lambda: up.align(model_fit, with_seg=False), args.replays)
    _, ms_acc = D.timed(lambda: up.accumulate(states, K, seg_f, sc_f), args.replays)
    fit.update(align_ms=HB.med(ms_al), align_without_seg_ms=HB.med(ms_al0), accumulate_ms=HB.med(ms_acc))
    ref_h = ref.cpu().numpy()
    t0 = time.perf_counter()
    clf = DiscreteHmmClassifier(S, K, args.n_iter, normalize=False).fit(ref_h, codes, lr_h)
    fit.update(classifier_fit_wall_ms=(time.perf_counter() - t0) * 1e3, classifier_rounds=clf.n_iter_)
    res["fit"] = fit

    # ---- the numpy restatement on every `sample`-th query ----
    (score_q, label_q), ms_p = D.timed(score_call(model_fit, sym_q, lq, dev, True), args.replays)
    sel = np.arange(0, qs.shape[0], args.sample)
    want_sym = R.tokenize(toks[K].codebook_, qs[sel].cpu().numpy(), lq_h[sel])
    t0 = time.perf_counter()
    want, wlab = R.score(R.Model(model_fit.emit, model_fit.stay, model_fit.adv, model_fit.n_states), want_sym, lq_h[sel])
    cpu_s = time.perf_counter() - t0
    res["numpy_restatement"] = dict(sampled_queries=int(len(sel)), sample_s=cpu_s, scaled_s=cpu_s * qs.shape[0] / len(sel),
                                    speedup=cpu_s * qs.shape[0] / len(sel) / (HB.med(ms_p) * 1e-3),
                                    sample_bits_equal=bool(
                                        np.array_equal(sym_q.cpu().numpy()[sel], want_sym)
                                        and np.array_equal(score_q.cpu().numpy()[sel].view(np.uint64), want.view(np.uint64))
                                        and np.array_equal(label_q.cpu().numpy()[sel], wlab)))
    if args.corpus > 0:
        res["accuracy"] = corpus_accuracy(args.corpus)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
