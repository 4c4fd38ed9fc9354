"""Writes tests/golden/nb_tree_golden.npz: GaussianNB() and DecisionTreeClassifier(random_state=42)
models fitted by scikit-learn on seeded Gaussian classes, with queries and scikit-learn's answers.

    python tests/golden/make_nb_tree_golden.py          # rewrite the file

Keys, per model name m in MODELS:
  m/classes; m/theta, m/var, m/class_prior (GaussianNB's fitted arrays);
  m/X [n, D], m/nb_pred, m/nb_jll (_joint_log_likelihood), m/tree_pred, m/tree_apply;
  m/tie_X [2, D], m/tie_pred, m/tie_jll: two Naive Bayes near ties;
  m/left, m/right, m/feature, m/threshold, m/leaf_class, m/max_depth (tree_'s arrays);
  m/bnd_X [4, D], m/bnd_pred, m/bnd_apply, m/bnd_node: four rows on a tree boundary.
one/...: a one-node tree (a single class) with its arrays, one/X, one/tree_pred, one/tree_apply.

A near tie is the end of a bisection in fp64 between two queries of different predicted class, run
until the midpoint equals an endpoint; pairs are tried until the top-two margin of the closer
endpoint is below 1e-14 (a few ulps of the scores), far below any rounding bound, so only
scikit-learn itself can label the row.

The boundary rows visit an internal node (m/bnd_node) whose threshold t lies below the middle of
the two float32 values f <= t < f' around it; their tested feature is, in order,
  f as float32 (the threshold itself when it is a float32; left), f' (one float32 ulp above; right),
  the float32 below f (left), and the double just above t, whose float32 cast is f <= t: left,
  although x > t -- the row that goes wrong if the cast is left out.

The script asserts, with the CPU restatement (tests/nb_tree_reference.py), that every ordinary
query's smallest Naive Bayes margin is at least 16 times the certificate's threshold, so that no
evaluation of the contract within the bound can leave an ordinary row uncertified.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "nb_tree_golden.npz")
# name: (labels, columns, training rows per class, spread of the class centres, queries)
MODELS = {
    "c2": ((0, 1), 3, 150, 1.0, 200),
    "c3": ((3, 7, 11), 40, 200, 0.35, 300),
    "c10": (tuple(range(10)), 15, 200, 0.8, 400),
}
TREE_KEYS = ("left", "right", "feature", "threshold", "leaf_class", "max_depth")


def _reference():
    tests = os.path.dirname(HERE)
    sys.path.insert(0, tests)
    try:
        import nb_tree_reference
    finally:
        sys.path.remove(tests)
    return nb_tree_reference


def make_data(name):
    labels, D, per, spread, nq = MODELS[name]
    rng = np.random.default_rng(2000 + len(labels))
    centres = rng.normal(0.0, spread, (len(labels), D))
    scale = rng.uniform(0.6, 1.5, (len(labels), D))
    X = np.concatenate([c + s * rng.normal(0.0, 1.0, (per, D)) for c, s in zip(centres, scale)])
    y = np.repeat(np.asarray(labels), per)
    order = rng.permutation(len(y))  # interleaved labels
    which = rng.integers(0, len(labels), nq)
    Q = centres[which] + scale[which] * rng.normal(0.0, 1.2, (nq, D))
    return X[order], y[order], Q


def fit(name):
    """(GaussianNB, DecisionTreeClassifier, queries) of a model name."""
    from sklearn.naive_bayes import GaussianNB
    from sklearn.tree import DecisionTreeClassifier
    X, y, Q = make_data(name)
    return GaussianNB().fit(X, y), DecisionTreeClassifier(random_state=42).fit(X, y), Q


def fit_one_node():
    from sklearn.tree import DecisionTreeClassifier
    rng = np.random.default_rng(77)
    X = rng.normal(0.0, 1.0, (20, 4))
    return DecisionTreeClassifier(random_state=42).fit(X, np.full(20, 5)), rng.normal(0.0, 1.0, (33, 4))


def margin(nb, x):
    j = np.sort(nb._joint_log_likelihood(x[None, :])[0])
    return j[-1] - j[-2]


def near_tie(nb, a, b):
    """Bisect between a and b (different predicted classes) until the midpoint is an endpoint;
    the endpoint with the smaller top-two margin."""
    pa = nb.predict(a[None, :])[0]
    assert pa != nb.predict(b[None, :])[0]
    while True:
        mid = 0.5 * (a + b)
        if np.array_equal(mid, a) or np.array_equal(mid, b):
            return a if margin(nb, a) <= margin(nb, b) else b
        if nb.predict(mid[None, :])[0] == pa:
            a = mid
        else:
            b = mid


def near_ties(nb, Q, want=2):
    pred = nb.predict(Q)
    out = []
    for i in range(len(Q) - 1):
        if pred[i] != pred[i + 1]:
            t = near_tie(nb, Q[i].copy(), Q[i + 1].copy())
            if margin(nb, t) < 1e-14:
                out.append(t)
                if len(out) == want:
                    return np.stack(out)
    raise AssertionError("no near ties found")


def boundary_rows(tree, Q):
    """Four rows through an internal node whose threshold is below the middle of its float32
    neighbours; (rows, node)."""
    t = tree.tree_
    paths = tree.decision_path(Q).toarray().astype(bool)
    for node in range(t.node_count):
        if t.children_left[node] == -1:
            continue
        thr, f = float(t.threshold[node]), int(t.feature[node])
        lo = np.float32(thr)
        if float(lo) > thr:
            lo = np.nextafter(lo, np.float32(-np.inf))
        hi = np.nextafter(lo, np.float32(np.inf))
        x_above = np.nextafter(thr, np.inf)
        if not (np.float32(x_above) == lo and x_above > thr):
            continue
        for base in np.flatnonzero(paths[:, node]):
            rows = np.repeat(Q[base][None, :], 4, axis=0)
            rows[:, f] = [float(lo), float(hi), float(np.nextafter(lo, np.float32(-np.inf))), x_above]
            if tree.decision_path(rows).toarray().astype(bool)[:, node].all():
                side = np.float32(rows[:, f]).astype(np.float64) <= thr
                assert side.tolist() == [True, False, True, True] and rows[3, f] > thr
                return rows, node
    raise AssertionError("no boundary node found")


def tree_part(R, tree, Q):
    a = R.tree_arrays(tree)
    out = {k: a[k] for k in TREE_KEYS}
    out["tree_pred"], out["tree_apply"] = tree.predict(Q).astype(np.int64), tree.apply(Q).astype(np.int64)
    return out


def build_model(R, name):
    nb, tree, Q = fit(name)
    m = {"theta": nb.theta_.copy(), "var": nb.var_.copy(), "class_prior": nb.class_prior_.copy(),
         "classes": np.asarray(nb.classes_, dtype=np.int64)}
    T = near_ties(nb, Q)
    B, node = boundary_rows(tree, Q)
    # every ordinary query is decided with room to spare, by the reference alone
    ratio = R.gnb_margin_ratio(R.gnb_jll(m, Q), R.gnb_bound(m, Q))
    assert ratio.min() >= 16.0, (name, ratio.min())
    m.update(X=Q, nb_pred=nb.predict(Q).astype(np.int64), nb_jll=nb._joint_log_likelihood(Q),
             tie_X=T, tie_pred=nb.predict(T).astype(np.int64), tie_jll=nb._joint_log_likelihood(T),
             bnd_X=B, bnd_pred=tree.predict(B).astype(np.int64), bnd_apply=tree.apply(B).astype(np.int64),
             bnd_node=np.int64(node))
    m.update(tree_part(R, tree, Q))
    return m


def build():
    R = _reference()
    g = {"%s/%s" % (name, k): v for name in MODELS for k, v in build_model(R, name).items()}
    tree, Q = fit_one_node()
    one = tree_part(R, tree, Q)
    one.update(X=Q, classes=np.asarray(tree.classes_, dtype=np.int64))
    g.update({"one/%s" % k: v for k, v in one.items()})
    return g


if __name__ == "__main__":
    g = build()
    np.savez_compressed(OUT, **g)
    R = _reference()
    for name in MODELS:
        m = {k: g["%s/%s" % (name, k)] for k in ("theta", "var", "class_prior")}
        ratio = R.gnb_margin_ratio(R.gnb_jll(m, g[name + "/X"]), R.gnb_bound(m, g[name + "/X"]))
        tj = np.sort(g[name + "/tie_jll"], axis=1)
        print(name, "nodes", len(g[name + "/left"]), "depth", int(g[name + "/max_depth"]), "min margin / threshold",
              ratio.min(), "tie margins", tj[:, -1] - tj[:, -2], "boundary node", int(g[name + "/bnd_node"]))
    print(OUT, os.path.getsize(OUT), "bytes")
