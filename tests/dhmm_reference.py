"""numpy restatement of csrc/dhmm.hip (include/dsp_audiorec.h: dsp_dhmm_score, dsp_dhmm_align,
dsp_dhmm_accumulate) and of the host side on it (DhmmModelSet, VqTokenizer, DiscreteHmmClassifier.fit); a
plain helper module like tests/hmm_reference.py: no test, no fixture.

Every value is defined bit for bit -- fp64 add and min in a fixed order, integer counts, the logarithms
only in ``build_model`` -- so everything here is compared with array_equal on raw bits.  The Viterbi pass
exists in two independent forms:
  "table"  an explicit per-frame, per-state np.float64 loop that stores the whole V table and walks it
           back, re-deriving a and b;
  "rows"   all sequences scored against one model advance together, one row at a time; it keeps one row
           of V and one direction bit per cell, and walks every sequence back at once.
"""
import numpy as np

import vq_reference as VQ

INF = np.float64(np.inf)
MAX_STATES, MAX_SYMBOLS = 32, 256


class Model:
    """A model set in the ABI's form: emit [C, Smax, K], stay, adv [C, Smax], n_states [C]."""

    def __init__(self, emit, stay, adv, n_states):
        self.emit, self.stay, self.adv = (np.asarray(v, np.float64) for v in (emit, stay, adv))
        self.n_states = np.asarray(n_states, np.int32)

    @property
    def K(self):
        return self.emit.shape[2]

    def one(self, c):
        """(emit [S, K], stay, adv [S]) of model c, or None when n_states is out of range."""
        S = int(self.n_states[c])
        if S < 1 or S > self.emit.shape[1]:
            return None
        return self.emit[c, :S], self.stay[c, :S], self.adv[c, :S]


def viterbi_table(sym, emit, stay, adv):
    """One pair, the per-cell loop over the symbols sym [n]: (score, seg int list of S entries or None when
    the score is +inf).  A symbol outside [0, K) gives +inf before the table is touched."""
    n, (S, K) = len(sym), emit.shape
    if any(int(k) < 0 or int(k) >= K for k in sym):
        return INF, None
    V = np.full((n, S), INF)
    for t in range(n):
        for s in range(S):
            e = np.float64(emit[s, int(sym[t])])
            if t == 0:
                V[t, s] = e if s == 0 else INF
            else:
                a = V[t - 1, s] + np.float64(stay[s])
                b = V[t - 1, s - 1] + np.float64(adv[s - 1]) if s > 0 else INF
                V[t, s] = e + (b if b < a else a)
    score = V[n - 1, S - 1]
    if not score < INF:
        return score, None
    seg, s = [0] * S, S - 1
    for t in range(n - 1, 0, -1):
        if s == 0:
            break
        a = V[t - 1, s] + stay[s]
        b = V[t - 1, s - 1] + adv[s - 1]
        if b < a:
            seg[s] = t
            s -= 1
    assert s == 0
    return score, seg


def viterbi_rows(sym, n, emit, stay, adv, ties=None):
    """All symbol rows sym [N, T] (lengths n, all in 1 .. T) under one model: (score [N], seg int32 [N, S],
    -1 rows where score is +inf).  ties: a two-entry list that collects [decided cells, of them a == b] --
    the cells (t >= 1, s >= 1, t < n) of clean rows whose min(a, b) is finite."""
    N, T = sym.shape
    S, K = emit.shape
    n = np.asarray(n, np.int64)
    tmax = int(n.max()) if N else 0
    live = np.arange(T)[None, :] < n[:, None]
    bad = (live & ((sym < 0) | (sym >= K))).any(axis=1)
    idx = np.clip(sym, 0, K - 1)  # never index the table with a symbol outside the alphabet
    V = np.full((N, S), INF)
    bits = np.zeros((tmax, N, S), bool)
    score = np.full(N, INF)
    for t in range(tmax):
        e = emit.T[idx[:, t]]  # [N, S]
        if t == 0:
            V = np.where(np.arange(S)[None, :] == 0, e, INF)
        else:
            a = V + stay[None, :]
            b = np.concatenate([np.full((N, 1), INF), V[:, :-1] + adv[None, :-1]], axis=1)
            bits[t] = b < a
            if ties is not None:
                cell = (~bad & (t < n))[:, None] & (np.arange(S)[None, :] >= 1) & (np.minimum(a, b) < INF)
                ties[0] += int(cell.sum())
                ties[1] += int((cell & (a == b)).sum())
            V = e + np.where(b < a, b, a)
        done = n - 1 == t
        score[done] = V[done, S - 1]
    score[bad] = INF
    ok = score < INF
    seg = np.zeros((N, S), np.int32)
    s = np.full(N, S - 1)
    rows = np.arange(N)
    for t in range(tmax - 1, 0, -1):
        step = ok & (t <= n - 1) & (s > 0) & bits[t, rows, s]
        seg[rows[step], s[step]] = t
        s = s - step
    assert (s[ok] == 0).all()
    seg[~ok] = -1
    return score, seg


def _valid_len(n, T):
    n = np.asarray(n, np.int64)
    return (n >= 1) & (n <= T)


def label_of(score):
    label = np.full(len(score), -1, np.int32)
    for i in range(len(score)):
        best = INF
        for c in range(score.shape[1]):
            if score[i, c] < best:
                best, label[i] = score[i, c], c
    return label


def score(model, sym, n, form="rows"):
    """dsp_dhmm_score: (score float64 [N, C], label int32 [N])."""
    N, T = sym.shape
    C = len(model.n_states)
    out = np.full((N, C), INF)
    ok = _valid_len(n, T)
    for c in range(C):
        m = model.one(c)
        if m is None or not ok.any():
            continue
        if form == "rows":
            out[ok, c] = viterbi_rows(sym[ok], np.asarray(n)[ok], *m)[0]
        else:
            for i in np.flatnonzero(ok):
                out[i, c] = viterbi_table(sym[i, :n[i]], *m)[0]
    return out, label_of(out)


def align(model, sym, n, start, members, form="rows", ties=None):
    """dsp_dhmm_align: (score float64 [P], seg int32 [P, Smax])."""
    N, T = sym.shape
    C, Smax = model.emit.shape[:2]
    members = np.asarray(members, np.int64)
    n = np.asarray(n, np.int64)
    P = len(members)
    out, seg = np.full(P, INF), np.full((P, Smax), -1, np.int32)
    for c in range(C):
        m = model.one(c)
        ps = np.arange(start[c], start[c + 1])
        if m is None or not len(ps):
            continue
        mem = members[ps]
        inr = (mem >= 0) & (mem < N)
        ok = inr.copy()
        ok[inr] = _valid_len(n[mem[inr]], T)
        ps, mem = ps[ok], mem[ok]
        if not len(ps):
            continue
        S = len(m[1])
        if form == "rows":
            sc, sg = viterbi_rows(sym[mem], n[mem], *m, ties=ties)
            out[ps], seg[ps, :S] = sc, sg
        else:
            for p, i in zip(ps, mem):
                sc, sg = viterbi_table(sym[i, :n[i]], *m)
                out[p] = sc
                if sg is not None:
                    seg[p, :S] = sg
    return out, seg


def uniform_seg(lengths, n_states, Smax):
    """The uniform start of a pair list: state s = frames s n // S .. (s + 1) n // S - 1; -1 rows for n < S."""
    seg = np.full((len(lengths), Smax), -1, np.int32)
    for p, (n, S) in enumerate(zip(lengths, n_states)):
        if n >= S:
            seg[p, :S] = [(s * int(n)) // int(S) for s in range(S)]
    return seg


def accumulate(n_states, K, sym, n, start, members, seg, score):
    """dsp_dhmm_accumulate: (cnt_emit int32 [C, Smax, K], cnt int32 [C, Smax], n_valid int32 [C], total [C])."""
    N, T = sym.shape
    C, Smax = len(n_states), seg.shape[1]
    cnt_emit, cnt = np.zeros((C, Smax, K), np.int32), np.zeros((C, Smax), np.int32)
    n_valid, total = np.zeros(C, np.int32), np.zeros(C)
    for c in range(C):
        S = int(n_states[c])
        if not 1 <= S <= Smax:
            continue
        tot = None
        for p in range(start[c], start[c + 1]):
            k = int(members[p])
            if not (0 <= k < N and 1 <= n[k] <= T):
                continue
            b = [int(v) for v in seg[p, :S]] + [int(n[k])]
            if b[0] != 0 or any(b[s] >= b[s + 1] for s in range(S)):
                continue
            row = sym[k, :n[k]]
            if ((row < 0) | (row >= K)).any():
                continue
            for s in range(S):
                for t in range(b[s], b[s + 1]):
                    cnt_emit[c, s, row[t]] += 1
                cnt[c, s] += b[s + 1] - b[s]
            tot = np.float64(score[p]) if tot is None else tot + np.float64(score[p])
            n_valid[c] += 1
        if tot is not None:
            total[c] = tot
    return cnt_emit, cnt, n_valid, total


def build_model(cnt_emit, cnt, n_valid, n_states, alpha, trans_floor, prev=None):
    """The host step (pipeline.DhmmModelSet), entry by entry: the only place with a logarithm."""
    C, Smax, K = cnt_emit.shape
    emit, stay, adv = np.zeros((C, Smax, K)), np.zeros((C, Smax)), np.zeros((C, Smax))
    alpha = np.float64(alpha)
    ak = alpha * np.float64(K)
    for c in range(C):
        for s in range(int(n_states[c])):
            den = np.float64(cnt[c, s]) + ak
            for k in range(K):
                emit[c, s, k] = -np.log((np.float64(cnt_emit[c, s, k]) + alpha) / den)
            if n_valid[c] == 0 and prev is not None:
                stay[c, s], adv[c, s] = prev.stay[c, s], prev.adv[c, s]
                continue
            p = np.float64(0.5)
            if n_valid[c] > 0 and cnt[c, s] > 0:
                p = (np.float64(cnt[c, s]) - np.float64(n_valid[c])) / np.float64(cnt[c, s])
            p = min(max(p, np.float64(trans_floor)), np.float64(1.0) - np.float64(trans_floor))
            stay[c, s], adv[c, s] = -np.log(p), -np.log(np.float64(1.0) - p)
    return Model(emit, stay, adv, n_states)


def tokenizer_fit(X, n, n_codes, n_iter=10, eps=0.01):
    """VqTokenizer.fit: ONE codebook [n_codes, F] trained on all sequences (tests/vq_reference.py's fit
    with all-equal labels)."""
    return VQ.fit(X, np.asarray(n), np.zeros(len(X), np.int64), n_codes, n_iter, eps)[0][0]


def tokenize(cb, X, n):
    """VqTokenizer.transform: sym int32 [N, T], -1 behind each sequence's frames."""
    N = len(X)
    return VQ.assign(cb[None], np.array([len(cb)], np.int32), X, np.asarray(n), [0, N], np.arange(N))[1]


def fit(X, n, codes, n_states, n_codes, n_iter=10, alpha=0.5, trans_floor=1e-3, vq_iter=10, eps=0.01):
    """DiscreteHmmClassifier.fit on already scaled padded sequences: (codebook, model, totals [rounds, C])."""
    C = int(codes.max()) + 1
    states = np.full(C, n_states, np.int32) if np.ndim(n_states) == 0 else np.asarray(n_states, np.int32)
    Smax = int(states.max())
    order = np.argsort(codes, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=C))])
    cb = tokenizer_fit(X, n, n_codes, vq_iter, eps)
    sym = tokenize(cb, X, n)
    seg = uniform_seg(n[order], states[codes[order]], Smax)
    st = accumulate(states, n_codes, sym, n, start, order, seg, np.zeros(len(order)))
    model = build_model(*st[:3], states, alpha, trans_floor)
    totals = []
    for _ in range(n_iter):
        sc, new_seg = align(model, sym, n, start, order)
        st = accumulate(states, n_codes, sym, n, start, order, new_seg, sc)
        totals.append(st[3])
        model = build_model(*st[:3], states, alpha, trans_floor, prev=model)
        same = np.array_equal(new_seg, seg)
        seg = new_seg
        if same:
            break
    return cb, model, np.array(totals, dtype=np.float64).reshape(len(totals), C)


# ---- test corpora ----
def dyadic_models(n_states, Smax, K, seed):
    """Costs that are small multiples of 1/8: every sum is exact, so many cells tie exactly."""
    rng = np.random.default_rng(seed)
    C = len(n_states)
    return Model(rng.integers(0, 4, (C, Smax, K)) / 8.0, rng.integers(0, 3, (C, Smax)) / 8.0,
                 rng.integers(0, 3, (C, Smax)) / 8.0, n_states)


def random_models(n_states, Smax, K, seed):
    """Real-valued models: emission rows drawn from a Dirichlet, p_stay in [0.2, 0.9]."""
    rng = np.random.default_rng(seed)
    C = len(n_states)
    b = rng.dirichlet(np.full(K, 0.7), (C, Smax))
    p = rng.uniform(0.2, 0.9, (C, Smax))
    with np.errstate(divide="ignore"):
        return Model(-np.log(b), -np.log(p), -np.log(1.0 - p), n_states)


GARBAGE = np.array([-1, 0, 2 ** 31 - 1, -2 ** 31], np.int64)  # 0 stands for K


def random_symbols(N, T, K, seed, lo=1, lengths=None):
    """sym int32 [N, T] uniform over the alphabet with lengths in lo .. T (or the given ones); behind each
    length the row holds garbage: -1, K, 2^31 - 1 and INT_MIN in turn."""
    rng = np.random.default_rng(seed)
    n = rng.integers(lo, T + 1, N).astype(np.int32) if lengths is None else np.asarray(lengths, np.int32)
    sym = rng.integers(0, K, (N, T)).astype(np.int64)
    junk = np.where(GARBAGE == 0, K, GARBAGE)[(np.arange(T)[None, :] + np.arange(N)[:, None]) % 4]
    behind = np.arange(T)[None, :] >= np.clip(n, 0, T)[:, None]
    return np.where(behind, junk, sym).astype(np.int32), n
