"""numpy restatement of csrc/dhmm_fb.hip (include/dsp_audiorec.h: dsp_dhmm_forward, dsp_dhmm_expect) and of
the host side on it (DhmmProbSet, dhmm_nll, DiscreteHmmClassifier.fit with training='baum_welch'); a plain
helper module like tests/dhmm_reference.py: no test, no fixture.

Every value is defined bit for bit -- fp64 multiply, add, max, frexp, ldexp and one division per frame in a
fixed order; the one logarithm is ``nll``'s -- so everything here is compared with array_equal on raw bits.
The forward and the backward pass exist in two independent forms:
  "loop"  an explicit per-frame, per-state loop of np.float64 scalars with np.frexp and np.ldexp, one pair
          at a time, every sequence swept over exactly its own frames;
  "rows"  all sequences of a model advance together one row at a time, vectorised; the backward rows of a
          sequence shorter than the longest are zeros until its own last frame.
"""
import itertools
from fractions import Fraction

import numpy as np

import dhmm_reference as DR

F0, F1 = np.float64(0.0), np.float64(1.0)


class Prob:
    """A model set in the ABI's form: pemit [C, Smax, K], pstay, padv [C, Smax], n_states [C]."""

    def __init__(self, pemit, pstay, padv, n_states):
        self.pemit, self.pstay, self.padv = (np.asarray(v, np.float64) for v in (pemit, pstay, padv))
        self.n_states = np.asarray(n_states, np.int32)

    def one(self, c):
        """(B [S, K], a, d [S]) of model c, or None when n_states is out of range."""
        S = int(self.n_states[c])
        if S < 1 or S > self.pemit.shape[1]:
            return None
        return self.pemit[c, :S], self.pstay[c, :S], self.padv[c, :S]


def _frexp_exp(m):
    return int(np.frexp(m)[1]) if m > 0 else 0


# ---- form "loop" ----
def forward_loop(sym, B, a, d):
    """One pair over the symbols sym [n]: (mant, expo, A [n, S]); (0.0, 0, None) for a symbol outside [0, K)."""
    n, (S, K) = len(sym), B.shape
    if n < 1 or any(int(k) < 0 or int(k) >= K for k in sym):
        return F0, 0, None
    A = np.zeros((n, S))
    E = 0
    for t in range(n):
        u = np.zeros(S)
        for s in range(S):
            e = np.float64(B[s, int(sym[t])])
            if t == 0:
                u[s] = e if s == 0 else F0
            else:
                p1 = A[t - 1, s] * np.float64(a[s])
                p2 = A[t - 1, s - 1] * np.float64(d[s - 1]) if s > 0 else F0
                u[s] = (p1 + p2) * e
        m = F0
        for s in range(S):
            m = u[s] if u[s] > m else m
        k = _frexp_exp(m)
        for s in range(S):
            A[t, s] = np.ldexp(u[s], -k)
        E += k
    v = A[n - 1, S - 1]
    if v == 0:
        return F0, 0, A
    f, k = np.frexp(v)
    return np.float64(f), E + int(k), A


def posterior_loop(sym, B, a, d, A):
    """The backward pass and the posteriors of one pair whose forward rows are A: (gamma [n, S], valid)."""
    n, S = A.shape
    gamma, valid = np.zeros((n, S)), True
    Bh = np.zeros(S)
    Bh[S - 1] = F1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for t in range(n - 1, -1, -1):
            if t < n - 1:
                o = int(sym[t + 1])
                w = np.zeros(S)
                for s in range(S):
                    w[s] = np.float64(a[s]) * (np.float64(B[s, o]) * Bh[s])
                    if s < S - 1:
                        w[s] = w[s] + np.float64(d[s]) * (np.float64(B[s + 1, o]) * Bh[s + 1])
                k = _frexp_exp(max(w))
                Bh = np.array([np.ldexp(w[s], -k) for s in range(S)])
            g = [A[t, s] * Bh[s] for s in range(S)]
            D = g[0]
            for s in range(1, S):
                D = D + g[s]
            r = F1 / D if D > 0 else np.float64(np.inf)
            if not r < np.inf:  # D_t == 0, or a subnormal D_t whose reciprocal overflows
                valid = False
                continue
            for s in range(S):
                gamma[t, s] = g[s] * r
    return gamma, valid


# ---- form "rows" ----
def _rescale(u):
    m = u.max(axis=1)
    k = np.where(m > 0, np.frexp(m)[1], 0).astype(np.int64)
    return np.ldexp(u, -k[:, None].astype(np.int32)), k


def forward_rows(sym, n, B, a, d, keep=False):
    """All symbol rows sym [N, T] (lengths n, all in 1 .. T) under one model: (mant [N], expo int32 [N], bad
    [N], A rows [tmax, N, S] or None)."""
    N, T = sym.shape
    S, K = B.shape
    n = np.asarray(n, np.int64)
    tmax = int(n.max()) if N else 0
    live = np.arange(T)[None, :] < n[:, None]
    bad = (live & ((sym < 0) | (sym >= K))).any(axis=1)
    idx = np.clip(sym, 0, K - 1)  # never index the table with a symbol outside the alphabet
    A, E = np.zeros((N, S)), np.zeros(N, np.int64)
    mant, expo = np.zeros(N), np.zeros(N, np.int64)
    rows = []
    for t in range(tmax):
        e = B.T[idx[:, t]]  # [N, S]
        if t == 0:
            u = np.where(np.arange(S)[None, :] == 0, e, 0.0)
        else:
            p1 = A * a[None, :]
            p2 = np.concatenate([np.zeros((N, 1)), A[:, :-1] * d[None, :-1]], axis=1)
            u = (p1 + p2) * e
        A, k = _rescale(u)
        E = E + k
        if keep:
            rows.append(A)
        done = n - 1 == t
        f, kk = np.frexp(A[done, S - 1])
        mant[done] = f
        expo[done] = np.where(f != 0, E[done] + kk, 0)
    mant[bad], expo[bad] = 0.0, 0
    return mant, expo.astype(np.int32), bad, (np.array(rows).reshape(tmax, N, S) if keep else None)


def posterior_rows(sym, n, B, a, d, A):
    """(gamma [N, tmax, S], every D_t > 0 with a finite reciprocal [N]) of the sequences whose forward rows are A [tmax, N, S]."""
    tmax, N, S = A.shape
    K = B.shape[1]
    n = np.asarray(n, np.int64)
    idx = np.clip(sym, 0, K - 1)
    Bh = np.zeros((N, S))
    gamma, valid = np.zeros((N, tmax, S)), np.ones(N, bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for t in range(tmax - 1, -1, -1):
            if t + 1 < tmax:
                x = B.T[idx[:, t + 1]] * Bh
                w = a[None, :] * x
                w[:, :-1] = w[:, :-1] + d[None, :-1] * x[:, 1:]
                Bh = _rescale(w)[0]
            Bh[n - 1 == t, S - 1] = 1.0  # every other entry of such a row is still zero
            g = A[t] * Bh
            D = g[:, 0].copy()
            for s in range(1, S):
                D = D + g[:, s]
            live = t < n
            r = 1.0 / D
            fine = (D > 0) & (r < np.inf)  # a subnormal D_t whose reciprocal overflows counts like D_t == 0
            valid &= ~live | fine
            use = live & fine
            gamma[use, t] = (g * r[:, None])[use]
    return gamma, valid


# ---- the entry points ----
def label_of(mant, expo):
    label = np.full(len(mant), -1, np.int32)
    for i in range(len(mant)):
        for c in range(mant.shape[1]):
            if mant[i, c] == 0:
                continue
            b = label[i]
            if b < 0 or expo[i, c] > expo[i, b] or (expo[i, c] == expo[i, b] and mant[i, c] > mant[i, b]):
                label[i] = c
    return label


def forward(model, sym, n, form="rows"):
    """dsp_dhmm_forward: (mant float64 [N, C], expo int32 [N, C], label int32 [N])."""
    N, T = sym.shape
    C = len(model.n_states)
    n = np.asarray(n, np.int64)
    mant, expo = np.zeros((N, C)), np.zeros((N, C), np.int32)
    ok = (n >= 1) & (n <= T)
    for c in range(C):
        m = model.one(c)
        if m is None or not ok.any():
            continue
        if form == "rows":
            mant[ok, c], expo[ok, c] = forward_rows(sym[ok], n[ok], *m)[:2]
        else:
            for i in np.flatnonzero(ok):
                mant[i, c], expo[i, c] = forward_loop(sym[i, :n[i]], *m)[:2]
    return mant, expo, label_of(mant, expo)


def expect(model, sym, n, start, members, form="rows"):
    """dsp_dhmm_expect: (mant [P], expo int32 [P], gamma [P, T, Smax], occ_emit [C, Smax, K], n_valid int32 [C],
    valid bool [P])."""
    N, T = sym.shape
    C, Smax, K = model.pemit.shape
    members, n = np.asarray(members, np.int64), np.asarray(n, np.int64)
    P = len(members)
    mant, expo, gamma = np.zeros(P), np.zeros(P, np.int32), np.zeros((P, T, Smax))
    occ, n_valid, valid = np.zeros((C, Smax, K)), np.zeros(C, np.int32), np.zeros(P, bool)
    for c in range(C):
        m = model.one(c)
        ps = np.arange(start[c], start[c + 1])
        if m is None or not len(ps):
            continue
        mem = members[ps]
        ok = (mem >= 0) & (mem < N)
        ok[ok] = (n[mem[ok]] >= 1) & (n[mem[ok]] <= T)
        ps, mem = ps[ok], mem[ok]
        if not len(ps):
            continue
        S = len(m[1])
        G = np.zeros((len(ps), S, K))
        if form == "rows":
            mant[ps], expo[ps], bad, A = forward_rows(sym[mem], n[mem], *m, keep=True)
            gm, good = posterior_rows(sym[mem], n[mem], *m, A)
            good &= ~bad & (mant[ps] != 0)
            gm[~good] = 0.0
            gamma[ps, :gm.shape[1], :S] = gm
            for t in range(gm.shape[1] - 1, -1, -1):  # descending t; a pair's own table, so no collision
                q = np.flatnonzero(good & (t < n[mem]))
                G[q, :, sym[mem[q], t]] = G[q, :, sym[mem[q], t]] + gm[q, t]
        else:
            good = np.zeros(len(ps), bool)
            for q, (p, i) in enumerate(zip(ps, mem)):
                row = sym[i, :n[i]]
                mant[p], expo[p], A = forward_loop(row, *m)
                if A is None or mant[p] == 0:
                    continue
                gm, good[q] = posterior_loop(row, *m, A)
                if not good[q]:
                    continue
                gamma[p, :n[i], :S] = gm
                for t in range(n[i] - 1, -1, -1):
                    for s in range(S):
                        G[q, s, row[t]] = G[q, s, row[t]] + gm[t, s]
        valid[ps] = good
        for q in np.flatnonzero(good):  # list order
            occ[c, :S] = occ[c, :S] + G[q]
        n_valid[c] = int(good.sum())
    return mant, expo, gamma, occ, n_valid, valid


def nll(mant, expo):
    """pipeline.dhmm_nll, entry by entry."""
    mant, expo = np.asarray(mant, np.float64), np.asarray(expo)
    out = np.full(mant.shape, np.inf)
    for i in np.ndindex(mant.shape):
        if mant[i] != 0:
            out[i] = -(np.log(mant[i]) + np.float64(expo[i]) * np.log(np.float64(2.0)))
    return out


def build_prob(occ_emit, n_valid, n_states, alpha=0.5, trans_floor=1e-3, prev=None):
    """The host step (pipeline.DhmmProbSet), entry by entry."""
    C, Smax, K = occ_emit.shape
    pemit, pstay, padv = np.zeros((C, Smax, K)), np.zeros((C, Smax)), np.zeros((C, Smax))
    alpha = np.float64(alpha)
    ak = alpha * np.float64(K)
    for c in range(C):
        for s in range(int(n_states[c])):
            occ = F0
            for k in range(K):
                occ = occ + np.float64(occ_emit[c, s, k])
            for k in range(K):
                pemit[c, s, k] = (np.float64(occ_emit[c, s, k]) + alpha) / (occ + ak)
            p = np.float64(0.5)
            if n_valid[c] == 0 and prev is not None:
                p = prev.pstay[c, s]
            else:
                if n_valid[c] > 0 and occ > 0:
                    p = (occ - np.float64(n_valid[c])) / occ
                p = min(max(p, np.float64(trans_floor)), F1 - np.float64(trans_floor))
            pstay[c, s], padv[c, s] = p, F1 - p
    return Prob(pemit, pstay, padv, n_states)


def to_costs(prob):
    """DhmmProbSet.to_costs as a dhmm_reference.Model."""
    C, Smax, K = prob.pemit.shape
    emit, stay, adv = np.zeros((C, Smax, K)), np.zeros((C, Smax)), np.zeros((C, Smax))
    with np.errstate(divide="ignore"):
        for c in range(C):
            for s in range(int(prob.n_states[c])):
                emit[c, s] = [-np.log(v) for v in prob.pemit[c, s]]
                stay[c, s], adv[c, s] = -np.log(prob.pstay[c, s]), -np.log(prob.padv[c, s])
    return DR.Model(emit, stay, adv, prob.n_states)


def fit(X, n, codes, n_states, n_codes, n_iter=10, alpha=0.5, trans_floor=1e-3, vq_iter=10, eps=0.01):
    """DiscreteHmmClassifier(training='baum_welch').fit on already scaled padded sequences: (codebook, prob,
    totals [n_iter, C])."""
    C = int(codes.max()) + 1
    states = np.full(C, n_states, np.int32) if np.ndim(n_states) == 0 else np.asarray(n_states, np.int32)
    Smax = int(states.max())
    order = np.argsort(codes, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=C))])
    cb = DR.tokenizer_fit(X, n, n_codes, vq_iter, eps)
    sym = DR.tokenize(cb, X, n)
    seg = DR.uniform_seg(n[order], states[codes[order]], Smax)
    st = DR.accumulate(states, n_codes, sym, n, start, order, seg, np.zeros(len(order)))
    prob = build_prob(st[0].astype(np.float64), st[2], states, alpha, trans_floor)
    totals = np.zeros((n_iter, C))
    for it in range(n_iter):
        mant, expo, _, occ, n_valid, _ = expect(prob, sym, n, start, order)
        cost = nll(mant, expo)
        for c in range(C):
            for p in range(start[c], start[c + 1]):
                if cost[p] < np.inf:
                    totals[it, c] = totals[it, c] + cost[p]
        prob = build_prob(occ, n_valid, states, alpha, trans_floor, prev=prob)
    return cb, prob, totals


# ---- independent checks ----
def brute_force(sym, B, a, d):
    """Exact likelihood and posteriors of one pair by enumerating every state path with fractions.Fraction:
    (likelihood, gamma [n][S] of Fractions or None when the likelihood is zero)."""
    n, S = len(sym), len(a)
    fr = Fraction
    total, through = fr(0), [[fr(0)] * S for _ in range(n)]
    if n >= S:
        for cuts in itertools.combinations(range(1, n), S - 1):  # the first frame of each state s >= 1
            state = [sum(1 for c in cuts if c <= t) for t in range(n)]
            p = fr(float(B[0, sym[0]]))
            for t in range(1, n):
                s = state[t]
                p *= (fr(float(a[s])) if state[t - 1] == s else fr(float(d[s - 1]))) * fr(float(B[s, sym[t]]))
            total += p
            for t in range(n):
                through[t][state[t]] += p
    if total == 0:
        return total, None
    return total, [[g / total for g in row] for row in through]


def log_forward(sym, B, a, d):
    """The log-domain forward pass with np.logaddexp: -log likelihood of one pair (symbols all in range)."""
    n, S = len(sym), len(a)
    with np.errstate(divide="ignore"):
        lB, la, ld = np.log(B), np.log(a), np.log(d)
    v = np.full(S, -np.inf)
    v[0] = lB[0, sym[0]]
    for t in range(1, n):
        w = v + la
        w[1:] = np.logaddexp(w[1:], v[:-1] + ld[:-1])
        v = w + lB[:, sym[t]]
    return -v[S - 1]


# ---- test corpora ----
def random_probs(n_states, Smax, K, seed, zeros=0.0):
    """Real-valued models: emission rows drawn from a Dirichlet, p_stay in [0.2, 0.9]; a share ``zeros`` of
    the emission entries and of the transitions set to 0.0."""
    rng = np.random.default_rng(seed)
    C = len(n_states)
    b = np.maximum(rng.dirichlet(np.full(K, 0.7), (C, Smax)), 2.0 ** -200)
    p = rng.uniform(0.2, 0.9, (C, Smax))
    q = 1.0 - p
    if zeros:
        b[rng.random(b.shape) < zeros] = 0.0
        p[rng.random(p.shape) < zeros / 2] = 0.0
        q[rng.random(q.shape) < zeros / 2] = 0.0
    return Prob(b, p, q, n_states)


def dyadic_probs(n_states, Smax, K, seed):
    """Probabilities that are multiples of 1/8 (0 included): every product along a path of n <= 8 frames has at
    most 45 significant bits, so the whole computation is exact."""
    rng = np.random.default_rng(seed)
    C = len(n_states)
    return Prob(rng.integers(0, 9, (C, Smax, K)) / 8.0, rng.integers(1, 9, (C, Smax)) / 8.0,
                rng.integers(1, 9, (C, Smax)) / 8.0, n_states)


TINY = 2.0 ** -300


def underflow_set():
    """A hand-made set of three 3-state models over two symbols with entries of 2^-300, and three symbol rows.
    Symbol 0 is certain in state 0 and has probability 2^-300 in states 1 and 2; symbol 1 the other way round;
    padv[0] = 2^-300.  Along a run of symbol 0 the row maximum stays in state 0, state 1 sits 2^-600 below it
    and state 2 a further padv[1] * 2^-300:
      model 0, padv[1] = 2^-150  state 2 sits near 2^-1050 below the maximum: a subnormal, non-zero cell;
      model 1, padv[1] = 2^-300  state 2 would sit 2^-1200 below: it underflows to zero;
      model 2                    model 0 with padv[1] = 2^-150 (1 + 2^-40) and p_stay = 3/8: the cell has bits
                                 below the subnormal grid, so it is rounded, not exact.
    Rows: (0, 0, 0) ends on that cell -- a subnormal result under models 0 and 2, zero likelihood under model
    1 although the path 0 -> 1 -> 2 exists; (0, 0, 0, 1, 1) passes it and ends on a normal cell (every D_t is
    normal, so the member is valid in dsp_dhmm_expect; the rows that END on the cell are not: 1 / D_{n-1} overflows); (0, 0, 0, 0, 0, 0) ends on it after several paths were
    added, each rounded into the subnormal grid.
    Returns (Prob, sym int32 [3, 6], len)."""
    B = np.array([[1.0, TINY], [TINY, 1.0], [TINY, 1.0]])
    pemit = np.stack([B, B, B])
    pstay = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.375, 0.375, 0.375]])
    padv = np.array([[TINY, 2.0 ** -150, 0.5], [TINY, TINY, 0.5],
                     [TINY, 2.0 ** -150 * (1 + 2.0 ** -40), 0.5]])
    sym = np.array([[0, 0, 0, -1, 2, 5], [0, 0, 0, 1, 1, -1], [0, 0, 0, 0, 0, 0]], np.int32)
    return Prob(pemit, pstay, padv, [3, 3, 3]), sym, np.array([3, 5, 6], np.int32)


def edge_lengths(n_states):
    """1, 2, S-1, S, S+1 of every model and 63 .. 65."""
    out = {1, 2, 63, 64, 65}
    for S in n_states:
        out |= {max(int(S) - 1, 1), int(S), int(S) + 1}
    return sorted(out)
