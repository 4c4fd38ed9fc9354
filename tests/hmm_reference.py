"""numpy restatement of csrc/hmm.hip (include/dsp_audiorec.h: dsp_hmm_score, dsp_hmm_align,
dsp_hmm_accumulate) and of the host side on it (HmmModelSet, the uniform start, HmmClassifier.fit).

Every value is defined bit for bit -- fp64 subtract, multiply, add, min and divide in a fixed order,
the logarithms only in ``build_model`` -- so everything here is compared with array_equal on raw bits.
The Viterbi pass exists in two independent forms:
  "table"  a per-cell loop that stores the whole V table and walks it back, re-deriving a and b;
  "rows"   vectorised over the states and over all sequences scored against one model; it keeps one
           row of V and one direction bit per cell, and walks every sequence back at once.  This is
           the form used for the long shapes.
"""
import numpy as np

INF = np.float64(np.inf)
MAX_STATES = 32


class Model:
    """A model set in the ABI's form: mean (mu), var, w [C, Smax, F], g, stay, adv [C, Smax], n_states [C]."""

    def __init__(self, mu, w, g, stay, adv, n_states, var=None):
        self.mu, self.w = np.asarray(mu, np.float64), np.asarray(w, np.float64)
        self.g, self.stay, self.adv = (np.asarray(v, np.float64) for v in (g, stay, adv))
        self.n_states = np.asarray(n_states, np.int32)
        self.var = None if var is None else np.asarray(var, np.float64)

    def one(self, c):
        """(mu [S, F], w [S, F], g, stay, adv [S]) of model c, or None when n_states is out of range."""
        S = int(self.n_states[c])
        if S < 1 or S > self.mu.shape[1]:
            return None
        return self.mu[c, :S], self.w[c, :S], self.g[c, :S], self.stay[c, :S], self.adv[c, :S]


def viterbi_table(x, mu, w, g, stay, adv):
    """One pair, the per-cell loop: (score, seg int list of S entries or None when score is +inf)."""
    n, F = x.shape
    S = len(g)
    V = np.full((n, S), INF)
    with np.errstate(invalid="ignore"):
        for t in range(n):
            for s in range(S):
                e = g[s]
                for f in range(F):
                    d = x[t, f] - mu[s, f]
                    e = e + w[s, f] * (d * d)
                if t == 0:
                    V[t, s] = e if s == 0 else INF
                else:
                    a = V[t - 1, s] + stay[s]
                    b = V[t - 1, s - 1] + adv[s - 1] if s > 0 else INF
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


def viterbi_rows(x, n, mu, w, g, stay, adv):
    """All sequences x [N, T, F] (lengths n, all in 1 .. T) under one model: (score [N], seg int32 [N, S],
    -1 rows where score is +inf), one row of V and the direction bits only."""
    N, T, F = x.shape
    S = len(g)
    n = np.asarray(n, np.int64)
    tmax = int(n.max()) if N else 0
    V = np.full((N, S), INF)
    bits = np.zeros((tmax, N, S), bool)
    score = np.full(N, INF)
    with np.errstate(invalid="ignore"):
        for t in range(tmax):
            e = np.broadcast_to(g, (N, S)).copy()
            for f in range(F):
                d = x[:, t, f, None] - mu[None, :, f]
                e = e + w[None, :, f] * (d * d)
            if t == 0:
                V = np.where(np.arange(S)[None, :] == 0, e, INF)
            else:
                a = V + stay[None, :]
                b = np.concatenate([np.full((N, 1), INF), V[:, :-1] + adv[None, :-1]], axis=1)
                bits[t] = b < a
                V = e + np.where(b < a, b, a)
            done = n - 1 == t
            score[done] = V[done, S - 1]
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


def score(model, x, n, form="rows"):
    """dsp_hmm_score: (score float64 [N, C], label int32 [N])."""
    N, T, F = x.shape
    C = len(model.n_states)
    out = np.full((N, C), INF)
    ok = _valid_len(n, T)
    for c in range(C):
        m = model.one(c)
        if m is None or not ok.any():
            continue
        if form == "rows":
            out[ok, c] = viterbi_rows(x[ok], np.asarray(n)[ok], *m)[0]
        else:
            for i in np.flatnonzero(ok):
                out[i, c] = viterbi_table(x[i, :n[i]], *m)[0]
    label = np.full(N, -1, np.int32)
    for i in range(N):
        best = INF
        for c in range(C):
            if out[i, c] < best:
                best, label[i] = out[i, c], c
    return out, label


def align(model, x, n, start, members, form="rows"):
    """dsp_hmm_align: (score float64 [P], seg int32 [P, Smax])."""
    N, T, F = x.shape
    C, Smax = model.mu.shape[:2]
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
        S = len(m[2])
        if form == "rows":
            sc, sg = viterbi_rows(x[mem], n[mem], *m)
            out[ps], seg[ps, :S] = sc, sg
        else:
            for p, i in zip(ps, mem):
                sc, sg = viterbi_table(x[i, :n[i]], *m)
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


def accumulate(mu_prev, var_prev, n_states, x, n, start, members, seg, score, var_floor):
    """dsp_hmm_accumulate: (mean, var [C, Smax, F], cnt int32 [C, Smax], n_valid int32 [C], total [C])."""
    N, T, F = x.shape
    C, Smax = mu_prev.shape[:2]
    mean, var = np.zeros((C, Smax, F)), np.zeros((C, Smax, F))
    cnt, n_valid, total = np.zeros((C, Smax), np.int32), np.zeros(C, np.int32), np.zeros(C)
    for c in range(C):
        S = int(n_states[c])
        accx = accq = None
        tot = np.float64(0.0)
        if 1 <= S <= Smax:
            for p in range(start[c], start[c + 1]):
                k = int(members[p])
                if not (0 <= k < N and 1 <= n[k] <= T):
                    continue
                b = [int(v) for v in seg[p, :S]] + [int(n[k])]
                if b[0] != 0 or any(b[s] >= b[s + 1] for s in range(S)):
                    continue
                X, Q = np.zeros((S, F)), np.zeros((S, F))
                for s in range(S):
                    fr = x[k, b[s]:b[s + 1]]
                    X[s], Q[s] = np.cumsum(fr, axis=0)[-1], np.cumsum(fr * fr, axis=0)[-1]
                    cnt[c, s] += b[s + 1] - b[s]
                if accx is None:
                    accx, accq, tot = X, Q, np.float64(score[p])
                else:
                    accx, accq, tot = accx + X, accq + Q, tot + np.float64(score[p])
                n_valid[c] += 1
        if accx is None:
            mean[c], var[c] = mu_prev[c], var_prev[c]
            continue
        k = cnt[c, :S, None].astype(np.float64)
        m = accx / k
        mean[c, :S] = m
        var[c, :S] = np.maximum(accq / k - m * m, var_floor)
        total[c] = tot
    return mean, var, cnt, n_valid, total


def build_model(mean, var, cnt, n_valid, n_states, trans_floor, prev=None):
    """The host step (pipeline.HmmModelSet), state by state: the only place with a logarithm."""
    C, Smax, F = mean.shape
    mu, vr, w = np.zeros((C, Smax, F)), np.zeros((C, Smax, F)), np.zeros((C, Smax, F))
    g, stay, adv = np.zeros((C, Smax)), np.zeros((C, Smax)), np.zeros((C, Smax))
    two_pi = 2.0 * np.pi
    for c in range(C):
        for s in range(int(n_states[c])):
            mu[c, s], vr[c, s] = mean[c, s], var[c, s]
            w[c, s] = 0.5 / var[c, s]
            acc = np.log(two_pi * var[c, s, 0])
            for f in range(1, F):
                acc = acc + np.log(two_pi * var[c, s, f])
            g[c, s] = 0.5 * acc
            if n_valid[c] == 0 and prev is not None:
                stay[c, s], adv[c, s] = prev.stay[c, s], prev.adv[c, s]
                continue
            p = np.float64(0.5)
            if n_valid[c] > 0 and cnt[c, s] > 0:
                p = (np.float64(cnt[c, s]) - np.float64(n_valid[c])) / np.float64(cnt[c, s])
            p = min(max(p, np.float64(trans_floor)), np.float64(1.0) - np.float64(trans_floor))
            stay[c, s], adv[c, s] = -np.log(p), -np.log(np.float64(1.0) - p)
    return Model(mu, w, g, stay, adv, n_states, var=vr)


def fit(X, n, codes, n_states, n_iter=10, var_floor=1e-3, trans_floor=1e-3):
    """HmmClassifier.fit on already scaled padded sequences: (model, totals [rounds, C])."""
    C, F = int(codes.max()) + 1, X.shape[2]
    states = np.full(C, n_states, np.int32) if np.ndim(n_states) == 0 else np.asarray(n_states, np.int32)
    Smax = int(states.max())
    order = np.argsort(codes, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=C))])
    seg = uniform_seg(n[order], states[codes[order]], Smax)
    zeros = np.zeros((C, Smax, F))
    st = accumulate(zeros, zeros, states, X, n, start, order, seg, np.zeros(len(order)), var_floor)
    model = build_model(*st[:4], states, trans_floor)
    totals = []
    for _ in range(n_iter):
        sc, new_seg = align(model, X, n, start, order)
        st = accumulate(model.mu, model.var, states, X, n, start, order, new_seg, sc, var_floor)
        totals.append(st[4])
        model = build_model(*st[:4], states, trans_floor, prev=model)
        same = np.array_equal(new_seg, seg)
        seg = new_seg
        if same:
            break
    return model, np.array(totals, dtype=np.float64).reshape(len(totals), C)


# ---- test corpora ----
def dyadic_models(C, Smax, F, seed, n_states=None):
    """Integer means in {0, 1, 2}, w = 0.5, g in {0, 1}, stay / adv in {0, 0.5, 1}: every sum is exact,
    so many cells tie exactly."""
    rng = np.random.default_rng(seed)
    S = rng.integers(1, Smax + 1, C) if n_states is None else np.asarray(n_states)
    m = Model(rng.integers(0, 3, (C, Smax, F)).astype(np.float64), np.full((C, Smax, F), 0.5),
              rng.integers(0, 2, (C, Smax)).astype(np.float64), rng.integers(0, 3, (C, Smax)) * 0.5,
              rng.integers(0, 3, (C, Smax)) * 0.5, S)
    return m


def dyadic_sequences(N, T, F, seed, lo=1):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 3, (N, T, F)).astype(np.float64), rng.integers(lo, T + 1, N).astype(np.int32)


def random_models(n_states, Smax, F, seed):
    """Real-valued models: means N(0, 1), variances in [0.2, 2], p_stay in [0.2, 0.9]."""
    rng = np.random.default_rng(seed)
    C = len(n_states)
    var = rng.uniform(0.2, 2.0, (C, Smax, F))
    p = rng.uniform(0.2, 0.9, (C, Smax))
    g = 0.5 * np.cumsum(np.log((2.0 * np.pi) * var), axis=2)[:, :, -1]
    return Model(rng.normal(0, 1, (C, Smax, F)), 0.5 / var, g, -np.log(p), -np.log(1.0 - p), n_states, var=var)


def tie_fraction(model, x, n):
    """Among the finite (sequence, model) pairs: the share whose walk back meets a finite tie a == b."""
    finite = tied = 0
    for c in range(len(model.n_states)):
        m = model.one(c)
        if m is None:
            continue
        mu, w, g, stay, adv = m
        S = len(g)
        for i in range(len(x)):
            xi = x[i, :n[i]]
            V = np.full((len(xi), S), INF)
            for t in range(len(xi)):
                e = g.copy()
                for f in range(xi.shape[1]):
                    d = xi[t, f] - mu[:, f]
                    e = e + w[:, f] * (d * d)
                if t == 0:
                    V[0, 0] = e[0]
                else:
                    a = V[t - 1] + stay
                    b = np.concatenate([[INF], V[t - 1, :-1] + adv[:-1]])
                    V[t] = e + np.minimum(a, b)
            if not V[-1, -1] < INF:
                continue
            finite += 1
            s, hit = S - 1, False
            for t in range(len(xi) - 1, 0, -1):
                if s == 0:
                    break
                a, b = V[t - 1, s] + stay[s], V[t - 1, s - 1] + adv[s - 1]
                hit = hit or (a == b and a < INF)
                if b < a:
                    s -= 1
            tied += hit
    return tied / max(finite, 1), finite
