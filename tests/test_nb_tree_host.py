"""CPU checks of Naive Bayes and Decision Tree prediction: the numpy restatements
(tests/nb_tree_reference.py) against scikit-learn -- the sequential fit bit for bit, the joint log
likelihood within the derived bound, the tree walk exactly --, the golden file's reproducibility,
the new exports, and the host side of TraditionalClassifier."""
import ctypes
import os
import sys

import numpy as np
import pytest

import nb_tree_reference as R
from conftest import GOLDEN

MODELS = ("c2", "c3", "c10")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "nb_tree_golden.npz"))


def nb_of(g, name):
    return {k: g["%s/%s" % (name, k)] for k in ("theta", "var", "class_prior", "classes")}


def tree_of(g, name):
    return {k: g["%s/%s" % (name, k)] for k in ("left", "right", "feature", "threshold", "leaf_class", "max_depth",
                                                "classes")}


def generator():
    sys.path.insert(0, GOLDEN)
    try:
        import make_nb_tree_golden
    finally:
        sys.path.remove(GOLDEN)
    return make_nb_tree_golden


def test_golden_covers_the_planned_models(golden):
    shapes = [(len(golden[n + "/classes"]), golden[n + "/theta"].shape[1]) for n in MODELS]
    assert shapes == [(2, 3), (3, 40), (10, 15)]
    assert golden["c3/classes"].tolist() == [3, 7, 11]
    for n in MODELS:
        D = golden[n + "/theta"].shape[1]
        assert 200 <= golden[n + "/X"].shape[0] <= 400 and golden[n + "/X"].shape[1] == D
        assert golden[n + "/tie_X"].shape == (2, D) and golden[n + "/bnd_X"].shape == (4, D)
        assert golden[n + "/nb_jll"].shape == (golden[n + "/X"].shape[0], len(golden[n + "/classes"]))
    assert len(golden["one/left"]) == 1 and int(golden["one/max_depth"]) == 0


@pytest.mark.parametrize("N,D,C", [(10, 2, 10), (257, 15, 2), (513, 17, 10), (3001, 40, 64), (300, 3, 3),
                                   (64, 7, 64), (500, 8, 5), (500, 9, 5), (400, 64, 4), (300, 200, 3)])
def test_sequential_fit_is_sklearns_bit_for_bit(N, D, C):
    from sklearn.naive_bayes import GaussianNB
    rng = np.random.default_rng(N + 7 * D + C)
    y = np.concatenate([np.arange(C), rng.integers(0, C, N - C)])
    rng.shuffle(y)
    X = rng.normal(0.0, 1.0, (N, D)) * rng.uniform(0.1, 10.0, D) + rng.normal(0.0, 3.0, D)
    m = GaussianNB().fit(X, y * 3 + 1)
    theta, var, count, eps = R.gnb_fit(X, y, C)
    assert np.array_equal(theta, m.theta_) and np.array_equal(var, m.var_)
    assert eps == m.epsilon_ and np.array_equal(count.astype(np.float64), m.class_count_)
    assert np.array_equal(count / count.sum(), m.class_prior_)


@pytest.mark.parametrize("name", MODELS)
def test_jll_restatement_within_the_derived_bound(golden, name):
    """The in-order sum against scikit-learn's pairwise one: within the bound, near ties included;
    equal argmax on the ordinary rows, all of them certifiable with a factor of 16 to spare; the
    near ties are not certifiable."""
    m = nb_of(golden, name)
    for X, want in ((golden[name + "/X"], golden[name + "/nb_jll"]), (golden[name + "/tie_X"], golden[name + "/tie_jll"])):
        jll, bound = R.gnb_jll(m, X), R.gnb_bound(m, X)
        assert np.all(np.abs(jll - want) <= bound), (np.abs(jll - want) / bound).max()
    X = golden[name + "/X"]
    jll, bound = R.gnb_jll(m, X), R.gnb_bound(m, X)
    assert np.array_equal(m["classes"][np.argmax(jll, axis=1)], golden[name + "/nb_pred"])
    assert R.gnb_margin_ratio(jll, bound).min() >= 16.0 and R.gnb_certified(jll, bound).all()
    T = golden[name + "/tie_X"]
    tj = np.sort(golden[name + "/tie_jll"], axis=1)
    assert np.all(tj[:, -1] - tj[:, -2] < 1e-14)
    assert not R.gnb_certified(R.gnb_jll(m, T), R.gnb_bound(m, T)).any()


@pytest.mark.parametrize("name", MODELS + ("one",))
def test_walk_restatement_is_sklearns(golden, name):
    t = tree_of(golden, name)
    pred, leaf = R.tree_walk(t, golden[name + "/X"])
    assert np.array_equal(leaf, golden[name + "/tree_apply"])
    assert np.array_equal(t["classes"][pred], golden[name + "/tree_pred"])
    if name != "one":
        B = golden[name + "/bnd_X"]
        pred, leaf = R.tree_walk(t, B)
        assert np.array_equal(leaf, golden[name + "/bnd_apply"]) and np.array_equal(t["classes"][pred], golden[name + "/bnd_pred"])
        # the fourth row: x > threshold as a double, left all the same
        node = int(golden[name + "/bnd_node"])
        f, thr = t["feature"][node], t["threshold"][node]
        assert B[3, f] > thr and float(np.float32(B[3, f])) <= thr


def test_walk_restatement_deep_tree_and_bad_rows():
    from sklearn.tree import DecisionTreeClassifier
    rng = np.random.default_rng(9)
    X = rng.normal(0.0, 1.0, (6000, 6))
    y = rng.integers(0, 4, 6000)  # noise: a deep tree
    tree = DecisionTreeClassifier(random_state=42).fit(X, y)
    t = R.tree_arrays(tree)
    Q = rng.normal(0.0, 1.0, (2000, 6))
    pred, leaf = R.tree_walk(t, Q)
    assert tree.tree_.max_depth > 15 and np.array_equal(leaf, tree.apply(Q))
    assert np.array_equal(t["classes"][pred], tree.predict(Q))
    Q[3, 2], Q[5, 0] = np.nan, 1e39
    pred, leaf = R.tree_walk(t, Q[:8])
    assert np.flatnonzero(leaf < 0).tolist() == [3, 5] and np.flatnonzero(pred < 0).tolist() == [3, 5]
    bad = dict(t)
    bad["right"] = t["right"].copy()
    bad["left"] = t["left"].copy()
    bad["left"][0], bad["right"][0] = 0, 0  # the root points at itself
    assert np.all(R.tree_walk(bad, Q[:3])[1] == -1)


def test_golden_regenerates_identically(golden):
    fresh = generator().build()
    assert sorted(fresh) == sorted(golden.files)
    for k in golden.files:
        assert np.array_equal(fresh[k], golden[k]), k


def test_exports_are_typed_and_check_their_arguments():
    from src import _hip
    lib = _hip.load_library()
    assert lib.dsp_abi_version() == 6 and _hip.ABI_VERSION == 6
    for name in ("dsp_gnb_fit", "dsp_gnb_workspace_bytes", "dsp_gnb_predict", "dsp_tree_workspace_bytes",
                 "dsp_tree_lds_nodes", "dsp_tree_predict"):
        assert name in _hip.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.dsp_gnb_fit.argtypes[5] is ctypes.c_double  # var_smoothing
    w = lib.dsp_gnb_workspace_bytes
    assert w(100, 15, 10) >= 4 + 2 * 100 * 10 * 8 and w(100, 4096, 64) > 0 and w(100, 1, 1) > 0
    assert w(100, 0, 10) == 0 and w(100, 4097, 10) == 0 and w(100, 15, 0) == 0 and w(100, 15, 65) == 0
    t = lib.dsp_tree_workspace_bytes
    assert t(1) >= 4 + 16 and t(5000) >= 4 + 16 * 5000 and t(0) == 0 and t(1 << 31) == 0
    assert lib.dsp_tree_lds_nodes() >= 1024
    # host argument checks come before any launch
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fit, E = lib.dsp_gnb_fit, _hip.DSP_ERR_ARGS
    assert fit(p, p, 10, 1, 2, 1e-9, p, p, p, p, p, 1 << 20, None) == E  # D = 1: numpy sums pairwise
    assert fit(p, p, 10, 4097, 2, 1e-9, p, p, p, p, p, 1 << 20, None) == E
    assert fit(p, p, 10, 3, 65, 1e-9, p, p, p, p, p, 1 << 20, None) == E
    assert fit(p, p, 0, 3, 2, 1e-9, p, p, p, p, p, 1 << 20, None) == E
    assert fit(p, p, 10, 3, 2, 1e-9, p, p, p, p, p, 8, None) == _hip.DSP_ERR_WORKSPACE
    pr = lib.dsp_gnb_predict
    assert pr(p, p, p, p, 0, 2, p, 4, p, None, p, p, 1 << 20, None) == E
    assert pr(p, p, p, p, 3, 65, p, 4, p, None, p, p, 1 << 20, None) == E
    assert pr(p, p, p, p, 3, 2, p, 4, p, None, p, None, 0, None) == _hip.DSP_ERR_WORKSPACE
    tp = lib.dsp_tree_predict
    assert tp(p, p, p, p, p, 0, 3, 4, p, 4, p, None, p, 1 << 20, None) == E
    assert tp(p, p, p, p, p, 5, -1, 4, p, 4, p, None, p, 1 << 20, None) == E
    assert tp(p, p, p, p, p, 5, 3, 4097, p, 4, p, None, p, 1 << 20, None) == E
    assert tp(p, p, p, p, p, 5, 3, 4, p, 4, p, None, None, 0, None) == _hip.DSP_ERR_WORKSPACE


def _data(seed, n=40, D=4):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.normal(-1, 1, (n, D)), rng.normal(1, 1, (n, D))]), np.repeat([2, 9], n)


@pytest.mark.parametrize("kind", ["naive_bayes", "decision_tree"])
def test_fit_needs_no_device_and_predict_raises_without_one(monkeypatch, kind):
    """fit on numpy rows is scikit-learn's; predict is an accelerated entry point: no quiet
    fall-back to the host."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from src import _hip
    from src.models import TraditionalClassifier
    X, y = _data(6)
    clf = TraditionalClassifier(kind).fit(X, y)
    assert np.array_equal(clf.model.predict(X), type(clf.model)(**clf.model.get_params()).fit(X, y).predict(X))
    with pytest.raises(_hip.HipError):
        clf.predict(X)
    if kind == "decision_tree":
        with pytest.raises(_hip.HipError):
            clf.apply(X)
    else:
        with pytest.raises(AttributeError):
            clf.apply(X)


def test_in_plan_decides_on_the_host(monkeypatch):
    """GnbIndex.in_plan / TreeIndex.in_plan ask no device: the ordinary fitted models are inside the plan;
    65 classes, a two-output tree, sparse rows and unfitted models are outside it, and predict then is
    scikit-learn's with the "off" record."""
    import torch
    from scipy.sparse import csr_matrix
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from src.models import TraditionalClassifier
    from src.pipeline import GnbIndex, TreeIndex
    X, y = _data(9)
    off = {'device': False, 'uncertified': 0}
    for kind, Index in (("naive_bayes", GnbIndex), ("decision_tree", TreeIndex)):
        clf = TraditionalClassifier(kind)
        assert not Index.in_plan(clf.model, X)  # not fitted
        clf.fit(X, y)
        assert Index.in_plan(clf.model, X) and not Index.in_plan(clf.model, csr_matrix(X))
    rng = np.random.default_rng(3)
    Xm, ym = rng.normal(0, 1, (130, 3)), np.arange(130) % 65
    many = TraditionalClassifier("naive_bayes").fit(Xm, ym)
    many.last_predict_stats = None
    assert not GnbIndex.in_plan(many.model, Xm) and GnbIndex.in_plan(many.model.fit(Xm, ym % 64), Xm)
    many.model.fit(Xm, ym)
    assert np.array_equal(many.predict(Xm), many.model.predict(Xm)) and many.last_predict_stats == off
    two = TraditionalClassifier("decision_tree")
    two.model.fit(X, np.stack([y, y[::-1]], axis=1))  # two outputs
    two.last_predict_stats = None
    assert not TreeIndex.in_plan(two.model, X)
    assert np.array_equal(two.predict(X), two.model.predict(X)) and two.last_predict_stats == off


def test_models_outside_the_plan_predict_through_sklearn(monkeypatch):
    """No device is touched: sparse rows, more than 64 classes, a multi-output tree."""
    import torch
    from scipy.sparse import csr_matrix
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from src.models import TraditionalClassifier
    X, y = _data(8)
    off = {'device': False, 'uncertified': 0}
    for kind in ("naive_bayes", "decision_tree"):
        clf = TraditionalClassifier(kind).fit(X, y)
        if kind == "decision_tree":  # (GaussianNB refuses sparse input itself)
            assert np.array_equal(clf.predict(csr_matrix(X)), clf.model.predict(X)) and clf.last_predict_stats == off
            assert np.array_equal(clf.apply(csr_matrix(X)), clf.model.apply(X))
    rng = np.random.default_rng(3)
    Xm, ym = rng.normal(0, 1, (130, 3)), np.arange(130) % 65
    clf = TraditionalClassifier("naive_bayes").fit(Xm, ym)
    assert np.array_equal(clf.predict(Xm), clf.model.predict(Xm)) and clf.last_predict_stats == off
    clf = TraditionalClassifier("decision_tree")
    clf.model.fit(X, np.stack([y, y[::-1]], axis=1))  # two outputs
    assert np.array_equal(clf.predict(X), clf.model.predict(X)) and clf.last_predict_stats == off
    assert np.array_equal(clf.apply(X), clf.model.apply(X))
