#!/usr/bin/env python
"""tools/dhmm_force_bench.py [--out profiles/dhmm_force_bench.json] [--corpus 2000] [--utterances 2000]
[--train-utterances 400] [--rate-utterances 10000] [--replays 5]: forced alignment and embedded training
(csrc/dhmm_force.hip).

The corpus and the utterances are tools/dhmm_decode_bench.py's: a DiscreteHmmClassifier (64 codewords, 5 states)
fitted on the isolated training sequences, an utterance the frame sequences of 2 to 6 test clips concatenated,
its transcript the clips' labels.

Everything is timed with device events, the median of --replays calls after two warm-up calls, on buffers made
once, all in this one process.  Reported:
  (i)   dsp_dhmm_force_align on the --utterances utterances with their true transcripts, with and without seg;
  (ii)  the same at the machine-filling shape: 64 models x 32 states, K = 64, --rate-utterances utterances of
        uniform random symbols (the corpus' lengths resampled), transcripts of 3 .. 5 words (those whose chain is
        longer than the utterance score +inf and still sweep every frame);
  (iii) dsp_dhmm_decode on the same symbols and the same model set in the same run, the yardstick: slot cells per
        second for both -- frames x slots x 64 lanes swept, and for the forced pass also frames x slots x
        transcript positions, the cells that belong to the chain;
  (iv)  one embedded training round on the corpus utterances: align + accumulate + the host rebuild, wall time;
  (v)   decode's word error rate on the test utterances after fit_connected on --train-utterances utterances built
        from the TRAINING clips, beside the same after the isolated fit on those clips, for a sweep of word_penalty;
  the numpy restatement (tests/dhmm_force_reference.py) on every --sample-th utterance, checked bit-equal."""
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
import dhmm_decode_bench as DD  # noqa: E402
import dtw_bench as D  # noqa: E402
import hmm_bench as HB  # noqa: E402


def force_call(models, sym, lens, trans, n_trans, enter, with_seg, dev):
    """The bare dsp_dhmm_force_align call on buffers made once."""
    from src import _hip
    lib = _hip.lib()
    (N, T), (C, Smax, K), Wmax = sym.shape, models.shape, trans.shape[1]
    margs = [_hip.ptr(t) for t in models.on_device(dev)]
    cost = torch.as_tensor(np.broadcast_to(np.asarray(enter, np.float64), (C,)).copy(), device=dev)
    score = torch.empty(N, dtype=torch.float64, device=dev)
    seg = torch.empty((N, Wmax, Smax), dtype=torch.int32, device=dev) if with_seg else None
    nbytes = lib.dsp_dhmm_force_workspace_bytes(C, N, T, Wmax, Smax, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call():
        _hip.check(lib.dsp_dhmm_force_align(*margs, _hip.ptr(cost), C, Smax, K, _hip.ptr(sym), _hip.ptr(lens), N, T,
                                            _hip.ptr(trans), _hip.ptr(n_trans), Wmax, _hip.ptr(score), _hip.ptr(seg),
                                            _hip.ptr(ws), nbytes, _hip.stream_handle(dev)), "dsp_dhmm_force_align")
        return score, seg
    return call


def padded(rows, width):
    out = np.full((len(rows), width), -1, np.int32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, np.array([len(r) for r in rows], np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dhmm_force_bench.json"))
    ap.add_argument("--corpus", type=int, default=2000)
    ap.add_argument("--utterances", type=int, default=2000)
    ap.add_argument("--train-utterances", type=int, default=400)
    ap.add_argument("--rate-utterances", type=int, default=10000)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--sample", type=int, default=100)
    ap.add_argument("--max-words", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dhmm_force_bench needs the MI355X: nothing is measured without it")
    import dhmm_force_reference as F
    import dhmm_reference as DR
    from src.models import DiscreteHmmClassifier, _as_padded, word_error_rate
    from src.pipeline import DhmmForceUpdater, DhmmModelSet
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0))

    # ---- the corpus, the isolated classifier, the utterances and their transcripts ----
    seqs, y = D.labelled_sequences(args.corpus, dev)
    perm = np.random.default_rng(0).permutation(len(y))
    tr, te = perm[:len(perm) * 8 // 10], perm[len(perm) * 8 // 10:]
    train_seqs, test_seqs = [seqs[i] for i in tr], [seqs[i] for i in te]
    clf = DiscreteHmmClassifier(n_states=5, n_codes=64).fit(train_seqs, y[tr])
    utts, ref = DD.utterances(test_seqs, y[te], args.utterances, seed=1)
    Xq, nq = _as_padded(utts, None)
    sym = clf.tokenizer_.transform(clf._scale(Xq, nq), nq)
    lens = torch.as_tensor(nq, device=dev)
    trans_h, ntr_h = padded([np.searchsorted(clf.classes_, r) for r in ref], 6)
    trans, n_trans = torch.as_tensor(trans_h, device=dev), torch.as_tensor(ntr_h, device=dev)
    frames, C = int(nq.sum()), len(clf.classes_)
    chain_cells = int((nq.astype(np.int64) * ntr_h).sum()) * 8
    res["corpus"] = dict(clips=len(y), train=len(tr), test=len(te), classes=C, n_states=5, n_codes=64, utterances=len(utts),
                         words_per_utterance=float(ntr_h.mean()), frames_per_utterance=float(nq.mean()))

    # ---- (i) the forced pass on the corpus utterances, (iii) the decoder beside it ----
    penalty = 20.0
    (score, seg), ms_seg = D.timed(force_call(clf.model_, sym, lens, trans, n_trans, penalty, True, dev), args.replays)
    _, ms_score = D.timed(force_call(clf.model_, sym, lens, trans, n_trans, penalty, False, dev), args.replays)
    _, ms_dec = D.timed(DD.decode_call(clf.model_, sym, lens, penalty, args.max_words, dev), args.replays)
    per = lambda cells, ms: cells / (HB.med(ms) * 1e-3)
    res["corpus_align"] = dict(N=len(utts), T=int(sym.shape[1]), frames=frames, models=C, slots=8, word_penalty=penalty,
                               finite=int(torch.isfinite(score).sum()),
                               with_seg_ms=HB.med(ms_seg), score_only_ms=HB.med(ms_score), decode_ms=HB.med(ms_dec),
                               with_seg_swept_cells_per_s=per(frames * 8 * 64, ms_seg),
                               score_only_swept_cells_per_s=per(frames * 8 * 64, ms_score),
                               with_seg_chain_cells_per_s=per(chain_cells, ms_seg),
                               decode_swept_cells_per_s=per(frames * 8 * 64, ms_dec),
                               decode_model_cells_per_s=per(frames * 8 * C, ms_dec))

    # ---- the numpy restatement on every `sample`-th utterance ----
    sel = np.arange(0, len(utts), args.sample)
    m = clf.model_
    t0 = time.perf_counter()
    want = F.align(DR.Model(m.emit, m.stay, m.adv, m.n_states), sym.cpu().numpy()[sel], nq[sel], trans_h[sel], ntr_h[sel],
                   np.full(C, penalty))
    cpu_s = time.perf_counter() - t0
    equal = (np.array_equal(score.cpu().numpy()[sel].view(np.uint64), want[0].view(np.uint64))
             and np.array_equal(seg.cpu().numpy()[sel], want[1]))
    res["numpy_restatement"] = dict(sampled_utterances=int(len(sel)), sample_s=cpu_s, scaled_s=cpu_s * len(utts) / len(sel),
                                    speedup=cpu_s * len(utts) / len(sel) / (HB.med(ms_seg) * 1e-3), sample_bits_equal=bool(equal))

    # ---- (iv) one embedded training round: align + accumulate + the host rebuild ----
    up = DhmmForceUpdater(sym, lens, trans, n_trans)
    states = np.full(C, 5, np.int32)
    rounds = []
    for _ in range(2 + args.replays):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc, sg = up.align(clf.model_, penalty)
        stats = up.accumulate(states, 64, sg)
        DhmmModelSet(*stats[:3], states, clf.alpha, clf.trans_floor, prev=clf.model_)
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) * 1e3)
    res["training_round"] = dict(N=len(utts), wall_ms=HB.med(rounds[2:]), valid=int(stats[3].sum()))

    # ---- (ii) and (iii) at the machine-filling shape: 64 models x 32 states, K = 64 ----
    rng = np.random.default_rng(2)
    N, K = args.rate_utterances, 64
    n_big = rng.choice(nq, N).astype(np.int32)
    T = int(n_big.max())
    sym_big = torch.as_tensor(rng.integers(0, K, (N, T)).astype(np.int32), device=dev)
    len_big = torch.as_tensor(n_big, device=dev)
    big = DB.random_model_set(64, 32, K, seed=3)
    ntr_big = rng.integers(3, 6, N).astype(np.int32)
    trans_big = torch.as_tensor(rng.integers(0, 64, (N, 5)).astype(np.int32), device=dev)
    fr = int(n_big.sum())
    swept, chain = fr * 32 * 64, int((n_big.astype(np.int64) * ntr_big).sum()) * 32
    ntr_dev = torch.as_tensor(ntr_big, device=dev)
    (score_big, _), ms_fs = D.timed(force_call(big, sym_big, len_big, trans_big, ntr_dev, 1.0, True, dev), args.replays)
    _, ms_f = D.timed(force_call(big, sym_big, len_big, trans_big, ntr_dev, 1.0, False, dev), args.replays)
    _, ms_d = D.timed(DD.decode_call(big, sym_big, len_big, 1.0, args.max_words, dev), args.replays)
    res["rate"] = dict(N=N, T=T, frames=fr, models=64, n_states=32, K=K, words_per_transcript=float(ntr_big.mean()),
                       finite=int(torch.isfinite(score_big).sum()),
                       force_with_seg_ms=HB.med(ms_fs), force_score_only_ms=HB.med(ms_f), decode_ms=HB.med(ms_d),
                       force_with_seg_swept_cells_per_s=per(swept, ms_fs), force_score_only_swept_cells_per_s=per(swept, ms_f),
                       force_with_seg_chain_cells_per_s=per(chain, ms_fs), decode_slot_cells_per_s=per(swept, ms_d),
                       swept_ratio_to_decode_with_seg=HB.med(ms_d) / HB.med(ms_fs),
                       swept_ratio_to_decode_score_only=HB.med(ms_d) / HB.med(ms_f),
                       note="swept cells count frames x 32 slots x 64 lanes for both kernels: every lane sweeps its slots "
                            "whether a word sits in it or not; chain cells count the transcript's positions only")

    # ---- (v) fit_connected on utterances of the training clips against the isolated fit on those clips ----
    train_utts, train_ref = DD.utterances(train_seqs, y[tr], args.train_utterances, seed=4)
    t0 = time.perf_counter()
    emb = DiscreteHmmClassifier(n_states=5, n_codes=64).fit_connected(train_utts, train_ref, word_penalty=penalty)
    fit_s = time.perf_counter() - t0
    rows = []
    for p in (0.0, 5.0, 10.0, 20.0, 40.0, 80.0):
        row = dict(word_penalty=p)
        for name, c in (("isolated_fit", clf), ("fit_connected", emb)):
            hyp, _ = c.decode(utts, word_penalty=p, max_words=args.max_words)
            row[name + "_word_error_rate"] = word_error_rate(ref, hyp)
            row[name + "_decoded_words_per_utterance"] = float(np.mean([len(h) for h in hyp]))
        rows.append(row)
    res["word_error_rate"] = dict(train_utterances=len(train_utts), train_word_penalty=penalty, fit_connected_s=fit_s,
                                  fit_connected_rounds=int(emb.n_iter_), fit_connected_totals=[float(v) for v in emb.totals_],
                                  isolated_fit_rounds=int(clf.n_iter_), test_utterances=len(utts), sweep=rows)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
