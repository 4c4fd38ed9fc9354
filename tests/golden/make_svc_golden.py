"""Writes tests/golden/svc_golden.npz: three SVC(C=1.0, kernel='rbf', random_state=42) models fitted
by scikit-learn on seeded 15-d Gaussian classes, with queries, SVC.predict, the one-vs-one
decision_function and two near-tie queries each.

    python tests/golden/make_svc_golden.py          # rewrite the file

Keys, per model name m in MODELS: m/sv, m/n_support, m/dual_coef, m/intercept, m/gamma, m/classes
(libsvm's arrays, scikit-learn's underscore attributes), m/X [n, 15], m/pred [n], m/dec (ovo, in
scikit-learn's signs: [n] and negated for two classes), m/tie_X [2, 15], m/tie_pred, m/tie_dec.

A near-tie query is the end of a bisection in fp64 between two queries on opposite sides of pair 0's
boundary, run until the midpoint equals an endpoint: |dec_0| is then 1e-16 .. 1e-15, far below any
rounding bound, so only libsvm itself can label it.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "svc_golden.npz")
D = 15
# name: (labels, training rows per class, spread of the class centres, queries)
MODELS = {
    "c2": ((0, 1), 200, 1.0, 64),
    "c3": ((3, 7, 11), 150, 1.6, 200),
    "c10": (tuple(range(10)), 160, 0.78, 600),
}


def make_data(name):
    labels, per, spread, nq = MODELS[name]
    rng = np.random.default_rng(1000 + len(labels))
    centres = rng.normal(0.0, spread, (len(labels), D))
    X = np.concatenate([c + rng.normal(0.0, 1.0, (per, D)) for c in centres])
    y = np.repeat(np.asarray(labels), per)
    which = rng.integers(0, len(labels), nq)
    Q = centres[which] + rng.normal(0.0, 1.2, (nq, D))
    return X, y, Q


def fit(name):
    from sklearn.svm import SVC
    X, y, Q = make_data(name)
    m = SVC(C=1.0, kernel='rbf', random_state=42).fit(X, y)
    m.decision_function_shape = 'ovo'  # read at call time: decision_function then reports the pairs
    return m, Q


def pair0(m, x):
    d = m.decision_function(x[None, :])
    return float(np.ravel(d)[0])


def near_tie(m, a, b):
    """Bisect between a and b (pair 0 of opposite signs) until the midpoint is an endpoint."""
    fa, fb = pair0(m, a), pair0(m, b)
    assert (fa > 0) != (fb > 0)
    steps = 0
    while True:
        mid = 0.5 * (a + b)
        if np.array_equal(mid, a) or np.array_equal(mid, b):
            return (a if abs(fa) <= abs(fb) else b), steps
        fm = pair0(m, mid)
        if (fm > 0) == (fa > 0):
            a, fa = mid, fm
        else:
            b, fb = mid, fm
        steps += 1


def build_model(name):
    m, Q = fit(name)
    C = len(m.classes_)
    nSV = m.support_vectors_.shape[0]
    d0 = np.asarray(m.decision_function(Q)).reshape(len(Q), -1)[:, 0]
    pos, neg = np.flatnonzero(d0 > 0), np.flatnonzero(d0 <= 0)
    ties = [near_tie(m, Q[pos[k]].copy(), Q[neg[k]].copy())[0] for k in range(2)]
    T = np.stack(ties)
    return {
        "sv": np.ascontiguousarray(m.support_vectors_, dtype=np.float64),
        "n_support": np.asarray(m._n_support, dtype=np.int32),
        "dual_coef": np.ascontiguousarray(m._dual_coef_, dtype=np.float64).reshape(C - 1, nSV),
        "intercept": np.asarray(m._intercept_, dtype=np.float64).reshape(C * (C - 1) // 2),
        "gamma": np.float64(m._gamma),
        "classes": np.asarray(m.classes_, dtype=np.int64),
        "X": Q, "pred": m.predict(Q).astype(np.int64), "dec": m.decision_function(Q),
        "tie_X": T, "tie_pred": m.predict(T).astype(np.int64), "tie_dec": m.decision_function(T),
    }


def build():
    return {"%s/%s" % (name, k): v for name in MODELS for k, v in build_model(name).items()}


if __name__ == "__main__":
    g = build()
    np.savez_compressed(OUT, **g)
    for name in MODELS:
        print(name, "nSV", g[name + "/sv"].shape[0], "n_support", g[name + "/n_support"].tolist(),
              "min |dec|", np.abs(g[name + "/dec"]).min(), "tie |dec0|",
              np.abs(g[name + "/tie_dec"].reshape(2, -1)[:, 0]))
    print(OUT, os.path.getsize(OUT), "bytes")
