"""numpy restatements of the contracts of dsp_gnb_fit, dsp_gnb_predict and dsp_tree_predict
(include/dsp_audiorec.h), for the CPU and GPU tests.

A Naive Bayes model is a dict: theta, var [C, D], class_prior [C], classes [C].
A tree is a dict: left, right, feature int32 [n], threshold float64 [n], leaf_class int32 [n],
max_depth, classes.
"""
import numpy as np

SAFETY = 4.0  # the certificate's factor (the SVC's)


# ---- fit ---------------------------------------------------------------------------------------
def seq_sum(A):
    """Column sums added in row order (np.cumsum never sums pairwise) to +0.0, np.add.reduce's start: a
    column of -0.0 alone sums to +0.0."""
    return np.cumsum(A, axis=0)[-1] + 0.0


def seq_mean_var(A):
    n = float(A.shape[0])
    mean = seq_sum(A) / n
    d = A - mean
    return mean, seq_sum(d * d) / n


def gnb_fit(X, codes, C, var_smoothing=1e-9):
    """(theta, var with epsilon, class_count int64, epsilon): every sum one sequential fp64 chain.  A class
    without rows has count 0 and NaN in its theta and var rows (0 / 0, include/dsp_audiorec.h)."""
    X = np.asarray(X, dtype=np.float64)
    D = X.shape[1]
    theta, var = np.empty((C, D)), np.empty((C, D))
    count = np.zeros(C, dtype=np.int64)
    for c in range(C):
        rows = X[codes == c]
        count[c] = len(rows)
        theta[c], var[c] = seq_mean_var(rows) if len(rows) else (np.nan, np.nan)
    eps = var_smoothing * seq_mean_var(X)[1].max()
    return theta, var + eps, count, eps


# ---- joint log likelihood ----------------------------------------------------------------------
def gnb_constants(m):
    """(log_prior, nconst) exactly as GaussianNB._joint_log_likelihood computes them."""
    return np.log(m["class_prior"]), -0.5 * np.sum(np.log(2.0 * np.pi * m["var"]), axis=1)


def gnb_q(m, X):
    """Q [Nq, C] = sum_d (x_d - theta_cd)^2 / var_cd, added in column order."""
    X = np.asarray(X, dtype=np.float64)
    Q = np.zeros((X.shape[0], m["theta"].shape[0]))
    with np.errstate(all="ignore"):
        for d in range(X.shape[1]):
            diff = X[:, d:d + 1] - m["theta"][None, :, d]
            Q = Q + (diff * diff) / m["var"][None, :, d]
    return Q


def gnb_jll(m, X):
    lp, nc = gnb_constants(m)
    with np.errstate(all="ignore"):
        return lp[None, :] + (nc[None, :] - 0.5 * gnb_q(m, X))


def gnb_bound(m, X):
    """[Nq, C] bound on |jll_a - jll_b| of two fp64 evaluations of the contract that differ in the
    order in which the D terms of Q are added.

    The terms t_d = (x_d - theta_d)^2 / var_d are the same correctly rounded sub, mul and div on
    both sides and are >= 0.  With u = 2^-53, a sum of D non-negative terms in any order is within
    (D - 1) u Q (1 + O(D u)) of Q, so the two sums differ by at most 2 (D - 1) u Q and the halves
    (exact) by (D - 1) u Q.  nconst - Q/2 adds one rounding of at most u (|nconst| + Q/2) on each
    side, log_prior + (.) one of at most u (|log_prior| + |nconst| + Q/2).  With
    M = |log_prior| + |nconst| + Q/2 that is below 2 (D + 1) u M; 2 (D + 8) u M leaves seven
    units for the second-order terms and for Q being the computed sum."""
    lp, nc = gnb_constants(m)
    D = m["theta"].shape[1]
    with np.errstate(all="ignore"):
        return 2.0 * (D + 8) * 2.0 ** -53 * (np.abs(lp)[None, :] + np.abs(nc)[None, :] + 0.5 * gnb_q(m, X))


def gnb_margin_ratio(jll, bound):
    """Per row: min over the other classes of (jll_w - jll_c) / (SAFETY (bound_w + bound_c)), w the
    first index of the largest score; certified iff > 1 (and every score finite).  inf for C = 1."""
    n, C = jll.shape
    w = np.argmax(jll, axis=1)
    r = np.arange(n)
    with np.errstate(all="ignore"):
        ratio = (jll[r, w][:, None] - jll) / (SAFETY * (bound[r, w][:, None] + bound))
    ratio[r, w] = np.inf
    return ratio.min(axis=1)


def gnb_certified(jll, bound):
    return np.all(np.isfinite(jll), axis=1) & (gnb_margin_ratio(jll, bound) > 1.0)


# ---- tree walk ---------------------------------------------------------------------------------
def tree_arrays(model):
    t = model.tree_
    return {"left": t.children_left.astype(np.int32), "right": t.children_right.astype(np.int32),
            "feature": t.feature.astype(np.int32), "threshold": t.threshold.astype(np.float64),
            "leaf_class": np.argmax(t.value[:, 0, :], axis=1).astype(np.int32),
            "max_depth": np.int64(t.max_depth), "classes": np.asarray(model.classes_)}


def tree_walk(t, X):
    """(pred class index, leaf): left iff (double)(float)x <= threshold; -1 for a row with a NaN or
    a value that is not finite as float32, for a walk longer than max_depth + 1 nodes and for a
    child index outside (node, n_nodes)."""
    with np.errstate(over="ignore"):
        V = np.asarray(X, dtype=np.float64).astype(np.float32)
    n_nodes, D = len(t["left"]), V.shape[1]
    ok = np.all(np.isfinite(V), axis=1)
    V = V.astype(np.float64)
    node = np.zeros(len(V), dtype=np.int64)
    leaf = np.full(len(V), -1, dtype=np.int64)
    live = ok.copy()
    for _ in range(int(t["max_depth"]) + 1):
        idx = np.flatnonzero(live)
        if not len(idx):
            break
        at = node[idx]
        is_leaf = t["left"][at] == -1
        leaf[idx[is_leaf]] = at[is_leaf]
        live[idx[is_leaf]] = False
        idx, at = idx[~is_leaf], at[~is_leaf]
        f = t["feature"][at]
        good = (f >= 0) & (f < D)
        live[idx[~good]] = False
        idx, at, f = idx[good], at[good], f[good]
        nxt = np.where(V[idx, f] <= t["threshold"][at], t["left"][at], t["right"][at])
        good = (nxt > at) & (nxt < n_nodes)
        live[idx[~good]] = False
        node[idx[good]] = nxt[good]
    pred = np.where(leaf >= 0, t["leaf_class"][np.maximum(leaf, 0)], -1)
    return pred.astype(np.int64), leaf
