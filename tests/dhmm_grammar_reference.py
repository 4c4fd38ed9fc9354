"""numpy restatement of csrc/dhmm_grammar.hip (include/dsp_audiorec.h: dsp_dhmm_decode_grammar), the one-pass
Viterbi over the word models of a discrete-HMM set under a word-pair grammar; a plain helper module like
tests/dhmm_decode_reference.py: no test, no fixture.

Every value is defined bit for bit -- fp64 add and compare in a fixed order -- so everything here is
compared with array_equal on raw bits.  The pass exists in two independent forms:
  "table"  the definition's per-cell loop: E, Bx and P of every (frame, model) stored, the (min, +) step a loop
           over the predecessors in ascending order with a strict compare, the words walked back over Bx and P;
  "rows"   all models and states of a frame advance together as [C, Smax] arrays, the (min, +) step is one
           broadcast [p, c] with argmin over p (the first of equal minima); no start is carried, only one
           direction bit per cell, and a word's first frame is recovered by walking the bits back from its exit.
A model with n_states outside 1 .. Smax is never a predecessor or a successor: the table form never touches its
tables or its cost rows and columns, the rows form masks them before any arithmetic.
"""
import numpy as np

import dhmm_decode_reference as R

INF = np.float64(np.inf)


def valid_models(model):
    S = model.n_states.astype(np.int64)
    return (S >= 1) & (S <= model.emit.shape[1])


def frames_table(row, model, enter, pair, leave):
    """(score, w, Bx [n, C], P [n, C]) by the per-cell loop; enter / leave None mean all 0.0."""
    n, C = len(row), len(model.n_states)
    ms = [model.one(c) for c in range(C)]
    live = [c for c in range(C) if ms[c] is not None]
    V = {c: np.full(len(ms[c][1]), INF) for c in live}
    st = {c: np.full(len(ms[c][1]), -1, np.int64) for c in live}
    G = {c: np.float64(0.0) + (np.float64(0.0) if enter is None else np.float64(enter[c])) for c in live}
    E = np.full((n, C), INF)
    Bx, P = np.full((n, C), -1, np.int64), np.full((n, C), -1, np.int64)
    for t in range(n):
        for c in live:
            emit, stay, adv = ms[c]
            S = len(stay)
            v, s0 = np.full(S, INF), np.full(S, -1, np.int64)
            for s in range(S):
                e = np.float64(emit[s, row[t]])
                a = V[c][s] + np.float64(stay[s])
                b = V[c][s - 1] + np.float64(adv[s - 1]) if s > 0 else G[c]
                if b < a:
                    v[s], s0[s] = e + b, (st[c][s - 1] if s > 0 else t)
                else:
                    v[s], s0[s] = e + a, st[c][s]
            V[c], st[c] = v, s0
            E[t, c], Bx[t, c] = v[-1], s0[-1]
        for c in live:
            best, arg = INF, -1
            for p in live:
                cand = E[t, p] + np.float64(pair[p, c])
                if cand < best:
                    best, arg = cand, p
            G[c], P[t, c] = best, arg
    score, w = INF, -1
    for c in live:
        cand = E[n - 1, c] + (np.float64(0.0) if leave is None else np.float64(leave[c]))
        if cand < score:
            score, w = cand, c
    return score, w, Bx, P


def frames_rows(row, model, enter, pair, leave, stats=None):
    """(score, w, bits [n, C, Smax], P [n, C]) with every model and state of a frame in one array operation.
    stats: a two-entry list that collects [finite G(t, c), of them the minimum shared by two or more
    predecessors]."""
    n = len(row)
    C, Smax, K = model.emit.shape
    S = model.n_states.astype(np.int64)
    okm = valid_models(model)
    valid = okm[:, None] & (np.arange(Smax)[None, :] < S[:, None])
    emit = np.where(valid[:, :, None], model.emit, INF)
    stay, adv = np.where(valid, model.stay, 0.0), np.where(valid, model.adv, 0.0)
    last = np.where(okm, S - 1, 0)
    ent = np.where(okm, np.zeros(C) if enter is None else np.asarray(enter, np.float64), INF)
    lv = np.where(okm, np.zeros(C) if leave is None else np.asarray(leave, np.float64), INF)
    pm = np.where(okm[:, None] & okm[None, :], np.asarray(pair, np.float64), INF)
    V = np.full((C, Smax), INF)
    G = np.float64(0.0) + ent
    bits = np.zeros((n, C, Smax), bool)
    P = np.full((n, C), -1, np.int64)
    cols = np.arange(C)
    for t in range(n):
        a = V + stay
        b = np.concatenate([G[:, None], V[:, :-1] + adv[:, :-1]], axis=1)
        bits[t] = (b < a) & valid
        V = np.where(valid, emit[:, :, row[t]] + np.where(b < a, b, a), INF)
        ex = np.where(okm, V[cols, last], INF)
        cand = ex[:, None] + pm  # [p, c]
        arg = np.argmin(cand, axis=0)  # the first of equal minima
        G = cand[arg, cols]
        P[t] = np.where(G < INF, arg, -1)
        if stats is not None:
            fin = G < INF
            stats[0] += int(fin.sum())
            stats[1] += int((((cand == G[None, :]).sum(axis=0) >= 2) & fin).sum())
    end = ex + lv
    w = int(np.argmin(end))
    if not end[w] < INF:
        return INF, -1, bits, P
    return end[w], w, bits, P


def decode_one(row, model, enter, pair, leave, form="rows", stats=None):
    """One clean utterance: (score, [(word, start) in time order]); the list is empty when no score is finite."""
    n = len(row)
    if form == "table":
        score, w, Bx, P = frames_table(row, model, enter, pair, leave)
        begin = lambda t, c: int(Bx[t, c])
    else:
        score, w, bits, P = frames_rows(row, model, enter, pair, leave, stats)
        begin = lambda t, c: R.begin_from_bits(bits, c, int(model.n_states[c]), t)
    if not score < INF:
        return INF, []
    out, t = [], n - 1
    while True:
        b = begin(t, w)
        out.append((w, b))
        if b == 0:
            break
        w, t = int(P[b - 1, w]), b - 1
    return score, out[::-1]


def decode(model, sym, n, enter, pair, leave, max_words=None, form="rows", stats=None):
    """dsp_dhmm_decode_grammar: (score float64 [N], n_words int32 [N], words, start int32 [N, max_words])."""
    N, T = sym.shape
    max_words = T if max_words is None else max_words
    score, n_words = np.full(N, INF), np.zeros(N, np.int32)
    words, start = np.full((N, max_words), -1, np.int32), np.full((N, max_words), -1, np.int32)
    for i in range(N):
        row = R._clean(sym[i], n[i], T, model.K)
        if row is None:
            continue
        sc, found = decode_one(row, model, enter, pair, leave, form, stats)
        score[i], n_words[i] = sc, len(found)
        for j, (w, b) in enumerate(found[:max_words]):
            words[i, j], start[i, j] = w, b
    return score, n_words, words, start


def forbidden_bigrams(words, n_words, enter, pair, leave):
    """How many outputs break the grammar: a first word with enter +inf, a bigram with pair +inf, a last word
    with leave +inf (rows cut short by max_words are checked as far as they go)."""
    bad = 0
    for i in range(len(n_words)):
        k = min(int(n_words[i]), words.shape[1])
        if k == 0:
            continue
        w = words[i, :k]
        bad += enter is not None and not enter[w[0]] < INF
        bad += int(sum(not pair[w[j], w[j + 1]] < INF for j in range(k - 1)))
        bad += leave is not None and k == n_words[i] and not leave[w[-1]] < INF
    return int(bad)


# ---- grammars and test corpora ----
def loop_grammar(enter, C):
    """Consequence (a): pair[p, c] = enter[c] for all p and leave NULL is dsp_dhmm_decode's free loop."""
    e = np.zeros(C) if enter is None else np.asarray(enter, np.float64)
    return e.copy(), np.tile(e[None, :], (C, 1)), None


def chain_grammar(words, enter, C):
    """Consequence (b): the grammar that admits exactly the transcript w_0 .. w_{L-1} of DISTINCT words: enter
    finite only at w_0, pair[w_{i-1}, w_i] = enter[w_i] and +inf elsewhere, leave 0.0 only at w_{L-1}."""
    e = np.zeros(C) if enter is None else np.asarray(enter, np.float64)
    first, pair, leave = np.full(C, INF), np.full((C, C), INF), np.full(C, INF)
    first[words[0]] = e[words[0]]
    for p, c in zip(words[:-1], words[1:]):
        pair[p, c] = e[c]
    leave[words[-1]] = 0.0
    return first, pair, leave


def tie_grammar(seed):
    """The dyadic grammar of the tie corpus (dhmm_decode_reference.tie_corpus(seed): ten models): pair in
    {0, 1/2, .. 2} with 30 % of its entries +inf, leave in {0, 1/2, 1}."""
    rng = np.random.default_rng(seed + 100)
    pair = rng.integers(0, 5, (10, 10)) / 2
    pair[rng.random((10, 10)) < 0.3] = INF
    leave = rng.integers(0, 3, 10) / 2
    return pair, leave


def random_grammar(C, seed, forbid=0.2):
    """Real-valued costs: enter, leave in [0, 3), pair in [0, 4) with a share ``forbid`` of +inf entries."""
    rng = np.random.default_rng(seed)
    pair = rng.uniform(0, 4, (C, C))
    pair[rng.random((C, C)) < forbid] = INF
    return rng.uniform(0, 3, C), pair, rng.uniform(0, 3, C)
