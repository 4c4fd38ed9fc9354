"""numpy restatement of csrc/dhmm_decode.hip (include/dsp_audiorec.h: dsp_dhmm_decode), the one-pass
Viterbi over a loop of the word models of a discrete-HMM set; a plain helper module like
tests/dhmm_reference.py: no test, no fixture.

Every value is defined bit for bit -- fp64 add and compare in a fixed order -- so everything here is
compared with array_equal on raw bits.  The pass exists in two independent forms:
  "table"  the definition's per-cell loop: V and start of every (frame, model, state) stored, X, W and B per
           frame, the words walked back over B;
  "rows"   all models and states of a frame advance together as [C, Smax] arrays; no start is carried, only
           one direction bit per cell, and a word's first frame is recovered by walking the bits back from
           its exit.
"""
import numpy as np

import dhmm_reference as D

INF = np.float64(np.inf)
MAX_MODELS = 64


def enter_of(model, enter):
    """The entry costs the recurrence uses: NULL is all 0.0, a model with an invalid n_states has +inf."""
    C, Smax = model.emit.shape[:2]
    cost = np.zeros(C) if enter is None else np.array(enter, np.float64)
    S = model.n_states.astype(np.int64)
    cost[(S < 1) | (S > Smax)] = INF
    return cost


def _clean(sym, n, T, K):
    """The utterance's n symbols, or None where the result is forced: a bad length or a symbol outside [0, K)."""
    n = int(n)
    if n < 1 or n > T:
        return None
    row = [int(k) for k in sym[:n]]
    return None if any(k < 0 or k >= K for k in row) else row


def frames_table(row, model, cost):
    """(X [n], W [n], B [n]) by the per-cell loop; models with cost +inf through an invalid n_states are
    never touched."""
    n, C = len(row), len(model.n_states)
    ms = [model.one(c) for c in range(C)]
    V = [[np.full(len(m[1]), INF) if m else None for m in ms]]
    st = [[np.full(len(m[1]), -1, np.int64) if m else None for m in ms]]
    X, W, B = np.full(n, INF), np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    xprev = np.float64(0.0)
    for t in range(n):
        Vt, stt = [], []
        for c in range(C):
            if ms[c] is None:
                Vt.append(None)
                stt.append(None)
                continue
            emit, stay, adv = ms[c]
            S = len(stay)
            v, s0 = np.full(S, INF), np.full(S, -1, np.int64)
            for s in range(S):
                e = np.float64(emit[s, row[t]])
                a = V[t][c][s] + np.float64(stay[s])
                b = V[t][c][s - 1] + np.float64(adv[s - 1]) if s > 0 else xprev + np.float64(cost[c])
                if b < a:
                    v[s], s0[s] = e + b, (st[t][c][s - 1] if s > 0 else t)
                else:
                    v[s], s0[s] = e + a, st[t][c][s]
            Vt.append(v)
            stt.append(s0)
        V.append(Vt)
        st.append(stt)
        best, w = INF, -1
        for c in range(C):
            if Vt[c] is not None and Vt[c][-1] < best:
                best, w = Vt[c][-1], c
        X[t], W[t] = best, w
        if w >= 0:
            B[t] = stt[w][-1]
        xprev = best
    return X, W, B


def frames_rows(row, model, cost, stats=None):
    """(X [n], W [n], bits [n, C, Smax]) with every model and state of a frame in one array operation.
    stats: a four-entry list that collects [decided cells, of them a == b, frames with a finite X, of them
    the minimum shared by two or more models] -- a decided cell is one of a valid state whose min(a, b) is
    finite."""
    n = len(row)
    C, Smax, K = model.emit.shape
    S = model.n_states.astype(np.int64)
    okm = (S >= 1) & (S <= Smax)
    valid = okm[:, None] & (np.arange(Smax)[None, :] < S[:, None])
    emit = np.where(valid[:, :, None], model.emit, INF)
    stay, adv = np.where(valid, model.stay, 0.0), np.where(valid, model.adv, 0.0)
    last = np.where(okm, S - 1, 0)
    V = np.full((C, Smax), INF)
    X, W = np.full(n, INF), np.full(n, -1, np.int64)
    bits = np.zeros((n, C, Smax), bool)
    xprev = np.float64(0.0)
    for t in range(n):
        a = V + stay
        b = np.concatenate([(xprev + cost)[:, None], V[:, :-1] + adv[:, :-1]], axis=1)
        bits[t] = (b < a) & valid
        V = np.where(valid, emit[:, :, row[t]] + np.where(b < a, b, a), INF)
        ex = np.where(okm, V[np.arange(C), last], INF)
        w = int(np.argmin(ex))  # the first of equal minima
        if ex[w] < INF:
            X[t], W[t] = ex[w], w
        if stats is not None:
            cell = valid & (np.minimum(a, b) < INF)
            stats[0] += int(cell.sum())
            stats[1] += int((cell & (a == b)).sum())
            if ex[w] < INF:
                stats[2] += 1
                stats[3] += int((ex == ex[w]).sum() >= 2)
        xprev = X[t]
    return X, W, bits


def begin_from_bits(bits, c, S, t):
    """The first frame of the word of model c (S states) that ends at frame t: walk the direction bits back
    from its last state."""
    s = S - 1
    while True:
        if bits[t, c, s]:
            if s == 0:
                return t
            s -= 1
        t -= 1


def decode_one(row, model, cost, form="rows", stats=None):
    """One clean utterance: (score, [(word, start, cum) in time order]); the list is empty when no word can
    end at the last frame."""
    n = len(row)
    if form == "table":
        X, W, B = frames_table(row, model, cost)
        begin = lambda t: int(B[t])
    else:
        X, W, bits = frames_rows(row, model, cost, stats)
        begin = lambda t: begin_from_bits(bits, int(W[t]), int(model.n_states[W[t]]), t)
    if not X[n - 1] < INF:
        return INF, []
    out, t = [], n - 1
    while t >= 0:
        b = begin(t)
        out.append((int(W[t]), b, X[t]))
        t = b - 1
    return X[n - 1], out[::-1]


def decode(model, sym, n, enter=None, max_words=None, form="rows", stats=None):
    """dsp_dhmm_decode: (score float64 [N], n_words int32 [N], words, start int32 [N, max_words], cum float64
    [N, max_words])."""
    N, T = sym.shape
    K = model.K
    max_words = T if max_words is None else max_words
    cost = enter_of(model, enter)
    score, n_words = np.full(N, INF), np.zeros(N, np.int32)
    words, start = np.full((N, max_words), -1, np.int32), np.full((N, max_words), -1, np.int32)
    cum = np.full((N, max_words), INF)
    for i in range(N):
        row = _clean(sym[i], n[i], T, K)
        if row is None:
            continue
        sc, found = decode_one(row, model, cost, form, stats)
        score[i], n_words[i] = sc, len(found)
        for j, (w, b, x) in enumerate(found[:max_words]):
            words[i, j], start[i, j], cum[i, j] = w, b, x
    return score, n_words, words, start, cum


# ---- test corpora ----
def tie_corpus(seed, N=24):
    """The dyadic tie corpus: C = 10 models of 1 .. 8 states (Smax = 8) over K = 16 symbols, emissions in
    {0, 1/2, .. 2}, stay / adv in {0, 1/2, 1}, enter in {0, 1/2, .. 2}; N utterances of 20 .. 64 frames.  Every
    sum is exact, so many cells and many exits tie exactly."""
    rng = np.random.default_rng(seed)
    states = np.array([1, 2, 3, 4, 5, 6, 7, 8, 3, 5], np.int32)
    model = D.Model(rng.integers(0, 5, (10, 8, 16)) / 2.0, rng.integers(0, 3, (10, 8)) / 2.0,
                    rng.integers(0, 3, (10, 8)) / 2.0, states)
    enter = rng.integers(0, 5, 10) / 2.0
    sym, n = D.random_symbols(N, 64, 16, seed + 1, lo=20)
    return model, enter, sym, n


def word_models(C, Smax, K, seed, states=None):
    """Real-valued models (dhmm_reference.random_models) with mixed n_states in 1 .. Smax unless given."""
    rng = np.random.default_rng(seed)
    if states is None:
        states = rng.integers(1, Smax + 1, C)
        states[rng.integers(0, C)] = Smax
    return D.random_models(np.asarray(states, np.int32), Smax, K, seed + 1)
