#!/usr/bin/env python
"""tools/dhmm_decode_bench.py [--out profiles/dhmm_decode_bench.json] [--corpus 2000] [--utterances 2000]
[--rate-utterances 10000] [--replays 5]: connected-word decoding (csrc/dhmm_decode.hip).

The corpus is tools/dhmm_bench.py's labelled one (--corpus host-synthesised clips, 10 labels, the 80 / 20 split of
vq_bench): a DiscreteHmmClassifier (64 codewords, 5 states) is fitted on the isolated training sequences, and an
utterance is the FRAME SEQUENCES of 2 to 6 test clips concatenated -- no new audio path, so there is no
coarticulation and no silence model; a word boundary is only a jump in the features.

Everything is timed with device events, the median of --replays calls after two warm-up calls, on buffers made
once, all in this one process.  Reported:
  the isolated accuracy on the test clips and the word error rate of the decoded utterances for a small sweep of
    word_penalty, with the mean number of decoded words per utterance (the reference has 4 on average);
  dsp_dhmm_decode on the --utterances utterances (10 models x 5 states, K = 64): the bare call on symbols already
    on the device, and DiscreteHmmClassifier.decode's wall time with scaling, tokenisation and downloads;
  the slot-cell rate at 64 models x 32 states x K = 64 x --rate-utterances utterances (uniform random symbols, the
    lengths of the corpus' utterances resampled), and dsp_dhmm_score's slot-cell rate on the same symbols and the
    same model set as the yardstick of this run: frames x 32 slots x 64 models over the call's time for both;
  the numpy restatement (tests/dhmm_decode_reference.py) on every --sample-th utterance, checked bit-equal."""
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

import dhmm_bench as DB  # noqa: E402
import dtw_bench as D  # noqa: E402
import hmm_bench as HB  # noqa: E402


def decode_call(models, sym, lens, enter, max_words, dev):
    """The bare dsp_dhmm_decode call on buffers made once."""
    from src import _hip
    lib = _hip.lib()
    (N, T), (C, Smax, K) = sym.shape, models.shape
    margs = [_hip.ptr(t) for t in models.on_device(dev)]
    cost = torch.as_tensor(np.broadcast_to(np.asarray(enter, np.float64), (C,)).copy(), device=dev)
    outs = [torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int32, device=dev),
            torch.empty((N, max_words), dtype=torch.int32, device=dev), torch.empty((N, max_words), dtype=torch.int32, device=dev),
            torch.empty((N, max_words), dtype=torch.float64, device=dev)]
    nbytes = lib.dsp_dhmm_decode_workspace_bytes(C, N, T, Smax, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call():
        _hip.check(lib.dsp_dhmm_decode(*margs, _hip.ptr(cost), C, Smax, K, _hip.ptr(sym), _hip.ptr(lens), N, T, max_words,
                                       *[_hip.ptr(o) for o in outs], _hip.ptr(ws), nbytes, _hip.stream_handle(dev)),
                   "dsp_dhmm_decode")
        return outs
    return call


def utterances(seqs, y, n, seed):
    """n utterances of 2 .. 6 of the sequences concatenated: (list of [frames, F] arrays, list of label lists)."""
    rng = np.random.default_rng(seed)
    utts, ref = [], []
    for _ in range(n):
        pick = rng.integers(0, len(seqs), int(rng.integers(2, 7)))
        utts.append(np.concatenate([seqs[i] for i in pick]))
        ref.append([int(y[i]) for i in pick])
    return utts, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dhmm_decode_bench.json"))
    ap.add_argument("--corpus", type=int, default=2000)
    ap.add_argument("--utterances", type=int, default=2000)
    ap.add_argument("--rate-utterances", type=int, default=10000)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--sample", type=int, default=100)
    ap.add_argument("--max-words", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dhmm_decode_bench needs the MI355X: nothing is measured without it")
    import dhmm_decode_reference as R
    import dhmm_reference as DR
    from src.models import DiscreteHmmClassifier, _as_padded, word_error_rate
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), isa_fp64_per_cell=dict(decode=4, dhmm=4))

    # ---- the corpus, the classifier, the utterances ----
    seqs, y = D.labelled_sequences(args.corpus, dev)
    perm = np.random.default_rng(0).permutation(len(y))
    tr, te = perm[:len(perm) * 8 // 10], perm[len(perm) * 8 // 10:]
    clf = DiscreteHmmClassifier(n_states=5, n_codes=64).fit([seqs[i] for i in tr], y[tr])
    test_seqs = [seqs[i] for i in te]
    iso = clf.classes_[np.argmin(clf.score_samples(test_seqs), axis=1)]
    utts, ref = utterances(test_seqs, y[te], args.utterances, seed=1)
    res["corpus"] = dict(clips=len(y), train=len(tr), test=len(te), classes=len(clf.classes_), n_states=5, n_codes=64,
                         fit_rounds=int(clf.n_iter_), isolated_accuracy=float(np.mean(iso == y[te])),
                         utterances=len(utts), words_per_utterance=float(np.mean([len(r) for r in ref])),
                         frames_per_utterance=float(np.mean([len(u) for u in utts])))
    sweep = []
    for penalty in (0.0, 5.0, 10.0, 20.0, 40.0, 80.0):
        t0 = time.perf_counter()
        hyp, _ = clf.decode(utts, word_penalty=penalty, max_words=args.max_words)
        wall = time.perf_counter() - t0
        sweep.append(dict(word_penalty=penalty, word_error_rate=word_error_rate(ref, hyp),
                          decoded_words_per_utterance=float(np.mean([len(h) for h in hyp])), decode_wall_ms=wall * 1e3))
    res["word_error_rate"] = sweep

    # ---- the decode call on the utterances' symbols ----
    Xq, nq = _as_padded(utts, None)
    sym = clf.tokenizer_.transform(clf._scale(Xq, nq), nq)
    lens = torch.as_tensor(nq, device=dev)
    frames = int(nq.sum())
    best = min(sweep, key=lambda r: r["word_error_rate"])["word_penalty"]
    outs, ms = D.timed(decode_call(clf.model_, sym, lens, best, args.max_words, dev), args.replays)
    res["decode"] = dict(N=len(utts), T=int(sym.shape[1]), frames=frames, models=10, n_states=5, K=64, word_penalty=best,
                         ms=HB.med(ms), slot_cells_per_s=frames * 8 * 10 / (HB.med(ms) * 1e-3),
                         frames_per_s=frames / (HB.med(ms) * 1e-3))

    # ---- the numpy restatement on every `sample`-th utterance ----
    sel = np.arange(0, len(utts), args.sample)
    m = clf.model_
    t0 = time.perf_counter()
    want = R.decode(DR.Model(m.emit, m.stay, m.adv, m.n_states), sym.cpu().numpy()[sel], nq[sel], np.full(10, best),
                    args.max_words)
    cpu_s = time.perf_counter() - t0
    got = [o.cpu().numpy()[sel] for o in outs]
    equal = all(np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, w.view(np.uint64) if w.dtype == np.float64 else w)
                for g, w in zip(got, want))
    res["numpy_restatement"] = dict(sampled_utterances=int(len(sel)), sample_s=cpu_s, scaled_s=cpu_s * len(utts) / len(sel),
                                    speedup=cpu_s * len(utts) / len(sel) / (HB.med(ms) * 1e-3), sample_bits_equal=bool(equal))

    # ---- the slot-cell rate at 64 models x 32 states, K = 64, and dsp_dhmm_score on the same symbols ----
    rng = np.random.default_rng(2)
    N, K = args.rate_utterances, 64
    n_big = rng.choice(nq, N).astype(np.int32)
    T = int(n_big.max())
    sym_big = torch.as_tensor(rng.integers(0, K, (N, T)).astype(np.int32), device=dev)
    len_big = torch.as_tensor(n_big, device=dev)
    big = DB.random_model_set(64, 32, K, seed=3)
    cells = int(n_big.sum()) * 32 * 64
    _, ms_d = D.timed(decode_call(big, sym_big, len_big, 1.0, args.max_words, dev), args.replays)
    _, ms_s = D.timed(DB.score_call(big, sym_big, len_big, dev, False), args.replays)
    rate_d, rate_s = cells / (HB.med(ms_d) * 1e-3), cells / (HB.med(ms_s) * 1e-3)
    res["rate"] = dict(N=N, T=T, frames=int(n_big.sum()), models=64, n_states=32, K=K, decode_ms=HB.med(ms_d),
                       decode_slot_cells_per_s=rate_d, dhmm_score_ms=HB.med(ms_s), dhmm_score_slot_cells_per_s=rate_s,
                       ratio_to_dhmm_score=rate_d / rate_s,
                       emission_bytes_per_s=rate_d * 8,
                       note="both rates count frames x 32 slots x 64 models; the decode reads 8 bytes of emissions per slot cell "
                            "from the table in the workspace, dsp_dhmm_score reads them from its LDS copy")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
