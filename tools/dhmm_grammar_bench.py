#!/usr/bin/env python
"""tools/dhmm_grammar_bench.py [--out profiles/dhmm_grammar_bench.json] [--corpus 2000] [--utterances 2000]
[--rate-utterances 10000] [--replays 5]: connected-word decoding under a word-pair grammar
(csrc/dhmm_grammar.hip), with §4.15's method.

The corpus and the classifier are tools/dhmm_decode_bench.py's: a DiscreteHmmClassifier (64 codewords, 5 states)
fitted on the isolated training sequences of the labelled host-synthesised clips.  An utterance is the frame
sequences of 2 to 6 test clips concatenated, but the WORD ORDER follows a sparse successor table: each word has
three allowed successors (drawn once, seed 5), the first word is uniform.  The training transcripts -- word
orders only, no audio -- are drawn from the same table with another seed.

Everything is timed with device events, the median of --replays calls after two warm-up calls, on buffers made
once, all in this one process.  Reported:
  the word error rate of the decoded utterances with grammar=None, with WordPairGrammar.from_transcripts of the
    training transcripts (alpha 0.5) and with WordPairGrammar.from_allowed of the true table, each for a small
    sweep of word_penalty, all in this run;
  dsp_dhmm_decode_grammar on the utterances' symbols (10 models x 5 states, K = 64, the bigram), and
    dsp_dhmm_decode on the same symbols and set: the yardstick, and the ratio of the two times;
  the same pair of calls at 64 models x 32 / 16 / 8 states x K = 64 x --rate-utterances utterances (uniform random
    symbols, the lengths of the corpus' utterances resampled, a random grammar with 30 % of pair forbidden);
  the numpy restatement (tests/dhmm_grammar_reference.py) on every --sample-th utterance of the first call and on
    four utterances of each of the large ones, checked bit-equal."""
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


def grammar_call(models, sym, lens, enter, pair, leave, max_words, dev):
    """The bare dsp_dhmm_decode_grammar call on buffers made once."""
    from src import _hip
    lib = _hip.lib()
    (N, T), (C, Smax, K) = sym.shape, models.shape
    margs = [_hip.ptr(t) for t in models.on_device(dev)]
    costs = [torch.as_tensor(np.ascontiguousarray(a, np.float64), device=dev) for a in (enter, pair, leave)]
    outs = [torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int32, device=dev),
            torch.empty((N, max_words), dtype=torch.int32, device=dev), torch.empty((N, max_words), dtype=torch.int32, device=dev)]
    nbytes = lib.dsp_dhmm_decode_grammar_workspace_bytes(C, N, T, Smax, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call():
        _hip.check(lib.dsp_dhmm_decode_grammar(*margs, *[_hip.ptr(c) for c in costs], C, Smax, K, _hip.ptr(sym), _hip.ptr(lens),
                                               N, T, max_words, *[_hip.ptr(o) for o in outs], _hip.ptr(ws), nbytes,
                                               _hip.stream_handle(dev)), "dsp_dhmm_decode_grammar")
        return outs
    return call


def successor_table(C, k, seed):
    """follows bool [C, C]: k allowed successors per word."""
    rng = np.random.default_rng(seed)
    follows = np.zeros((C, C), bool)
    for p in range(C):
        follows[p, rng.permutation(C)[:k]] = True
    return follows


def word_orders(follows, n, seed):
    """n word-index sequences of 2 .. 6 words: the first uniform, each next one uniform over its allowed successors."""
    rng = np.random.default_rng(seed)
    C = len(follows)
    out = []
    for _ in range(n):
        w = [int(rng.integers(0, C))]
        for _ in range(int(rng.integers(2, 7)) - 1):
            w.append(int(rng.choice(np.flatnonzero(follows[w[-1]]))))
        out.append(w)
    return out


def utterances(seqs, codes, orders, seed):
    """Each word order as the concatenation of one random sequence per word."""
    rng = np.random.default_rng(seed)
    of = [np.flatnonzero(codes == c) for c in range(int(codes.max()) + 1)]
    return [np.concatenate([seqs[int(rng.choice(of[w]))] for w in order]) for order in orders]


def bits_equal(got, want):
    return bool(all(np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, w.view(np.uint64) if w.dtype == np.float64 else w)
                    for g, w in zip(got, want)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dhmm_grammar_bench.json"))
    ap.add_argument("--corpus", type=int, default=2000)
    ap.add_argument("--utterances", type=int, default=2000)
    ap.add_argument("--rate-utterances", type=int, default=10000)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--sample", type=int, default=100)
    ap.add_argument("--max-words", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dhmm_grammar_bench needs the MI355X: nothing is measured without it")
    import dhmm_grammar_reference as GR
    import dhmm_reference as DR
    from src.models import DiscreteHmmClassifier, WordPairGrammar, _as_padded, word_error_rate
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0))

    # ---- the corpus, the classifier, the grammar, the utterances ----
    seqs, y = D.labelled_sequences(args.corpus, dev)
    perm = np.random.default_rng(0).permutation(len(y))
    tr, te = perm[:len(perm) * 8 // 10], perm[len(perm) * 8 // 10:]
    clf = DiscreteHmmClassifier(n_states=5, n_codes=64).fit([seqs[i] for i in tr], y[tr])
    C = len(clf.classes_)
    follows = successor_table(C, 3, seed=5)
    train_orders = word_orders(follows, args.utterances, seed=6)
    ref = word_orders(follows, args.utterances, seed=7)
    utts = utterances([seqs[i] for i in te], np.searchsorted(clf.classes_, y[te]), ref, seed=8)
    bigram = WordPairGrammar.from_transcripts(train_orders, C, alpha=0.5)
    syntax = WordPairGrammar.from_allowed(follows)
    res["corpus"] = dict(clips=len(y), train=len(tr), test=len(te), classes=C, n_states=5, n_codes=64, successors_per_word=3,
                         training_transcripts=len(train_orders), utterances=len(utts),
                         words_per_utterance=float(np.mean([len(r) for r in ref])),
                         frames_per_utterance=float(np.mean([len(u) for u in utts])))
    sweep = []
    for name, grammar in (("none", None), ("bigram", bigram), ("allowed", syntax)):
        for penalty in (0.0, 5.0, 10.0, 20.0, 40.0):
            hyp, _ = clf.decode(utts, word_penalty=penalty, max_words=args.max_words, grammar=grammar)
            hyp = [np.searchsorted(clf.classes_, h) for h in hyp]
            sweep.append(dict(grammar=name, word_penalty=penalty, word_error_rate=word_error_rate(ref, hyp),
                              decoded_words_per_utterance=float(np.mean([len(h) for h in hyp]))))
    res["word_error_rate"] = sweep
    res["best_word_error_rate"] = {name: min(r["word_error_rate"] for r in sweep if r["grammar"] == name)
                                   for name in ("none", "bigram", "allowed")}

    # ---- the two calls on the utterances' symbols ----
    Xq, nq = _as_padded(utts, None)
    sym = clf.tokenizer_.transform(clf._scale(Xq, nq), nq)
    lens = torch.as_tensor(nq, device=dev)
    frames = int(nq.sum())
    best = min((r for r in sweep if r["grammar"] == "bigram"), key=lambda r: r["word_error_rate"])["word_penalty"]
    g = bigram.plus(best)
    outs, ms_g = D.timed(grammar_call(clf.model_, sym, lens, g.enter, g.pair, g.leave, args.max_words, dev), args.replays)
    _, ms_d = D.timed(DD.decode_call(clf.model_, sym, lens, best, args.max_words, dev), args.replays)
    res["decode"] = dict(N=len(utts), T=int(sym.shape[1]), frames=frames, models=C, n_states=5, K=64, word_penalty=best,
                         grammar_ms=HB.med(ms_g), loop_decoder_ms=HB.med(ms_d), ratio_to_loop_decoder=HB.med(ms_g) / HB.med(ms_d),
                         frames_per_s=frames / (HB.med(ms_g) * 1e-3))

    # ---- the numpy restatement on every `sample`-th utterance ----
    sel = np.arange(0, len(utts), args.sample)
    m = clf.model_
    t0 = time.perf_counter()
    want = GR.decode(DR.Model(m.emit, m.stay, m.adv, m.n_states), sym.cpu().numpy()[sel], nq[sel], g.enter, g.pair, g.leave,
                     args.max_words)
    cpu_s = time.perf_counter() - t0
    res["numpy_restatement"] = dict(sampled_utterances=int(len(sel)), sample_s=cpu_s, scaled_s=cpu_s * len(utts) / len(sel),
                                    speedup=cpu_s * len(utts) / len(sel) / (HB.med(ms_g) * 1e-3),
                                    sample_bits_equal=bits_equal([o.cpu().numpy()[sel] for o in outs], want))

    # ---- 64 models x 32 / 16 / 8 states, K = 64 ----
    rng = np.random.default_rng(2)
    N, K = args.rate_utterances, 64
    n_big = rng.choice(nq, N).astype(np.int32)
    T = int(n_big.max())
    sym_host = rng.integers(0, K, (N, T)).astype(np.int32)
    sym_big, len_big = torch.as_tensor(sym_host, device=dev), torch.as_tensor(n_big, device=dev)
    enter, pair, leave = GR.random_grammar(64, seed=4, forbid=0.3)
    res["rate"] = []
    for S in (32, 16, 8):
        big = DB.random_model_set(64, S, K, seed=3)
        outs, ms_g = D.timed(grammar_call(big, sym_big, len_big, enter, pair, leave, args.max_words, dev), args.replays)
        _, ms_d = D.timed(DD.decode_call(big, sym_big, len_big, 1.0, args.max_words, dev), args.replays)
        cells = int(n_big.sum()) * S * 64
        want = GR.decode(DR.Model(big.emit, big.stay, big.adv, big.n_states), sym_host[:4], n_big[:4], enter, pair, leave,
                         args.max_words)
        res["rate"].append(dict(N=N, T=T, frames=int(n_big.sum()), models=64, n_states=S, K=K, grammar_ms=HB.med(ms_g),
                                loop_decoder_ms=HB.med(ms_d), ratio_to_loop_decoder=HB.med(ms_g) / HB.med(ms_d),
                                grammar_slot_cells_per_s=cells / (HB.med(ms_g) * 1e-3),
                                grammar_ns_per_frame=HB.med(ms_g) * 1e6 / int(n_big.sum()),
                                sample_bits_equal=bits_equal([o.cpu().numpy()[:4] for o in outs], want)))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
