"""Naive Bayes and Decision Tree on the MI355X (csrc/gnb.hip, csrc/tree.hip) against scikit-learn:
dsp_gnb_fit bit for bit, dsp_gnb_predict on the golden models (tests/golden/nb_tree_golden.npz) with
its certificate and the near ties, dsp_tree_predict on the golden, boundary, deep and malformed
trees, and the Python surface (gaussian_nb_fit, GnbIndex, TreeIndex, TraditionalClassifier).

The tolerance on jll is the derived bound of tests/nb_tree_reference.gnb_bound,
computed on the CPU from the model and the queries; everything else is compared exactly."""
import os
import sys

import numpy as np
import pytest
import torch

import nb_tree_reference as R
import predict_path_cases as cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODELS = ("c2", "c3", "c10")
TREE_KEYS = ("left", "right", "feature", "threshold", "leaf_class", "max_depth", "classes")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "nb_tree_golden.npz"))


def nb_of(g, name):
    return {k: g["%s/%s" % (name, k)] for k in ("theta", "var", "class_prior", "classes")}


def tree_of(g, name):
    return {k: g["%s/%s" % (name, k)] for k in TREE_KEYS}


def sk_models(name):
    """The scikit-learn models the golden file was made from, refitted (make_nb_tree_golden.py)."""
    sys.path.insert(0, GOLDEN)
    try:
        import make_nb_tree_golden
    finally:
        sys.path.remove(GOLDEN)
    return make_nb_tree_golden.fit(name)


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def _stream():
    from src import _hip
    return _hip.stream_handle(torch.device(DEV))


# ---- dsp_gnb_fit ---------------------------------------------------------------------------------
def abi_fit(X, codes, C, var_smoothing=1e-9):
    from src import _hip
    N, D = X.shape
    Xd, yd = _dev(X, torch.float64), _dev(codes, torch.int32)
    theta = torch.full((C, D), float("nan"), dtype=torch.float64, device=DEV)
    var = torch.full((C, D), float("nan"), dtype=torch.float64, device=DEV)
    count = torch.full((C,), -1, dtype=torch.int64, device=DEV)
    eps = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.empty(max(8 * D, 8), dtype=torch.uint8, device=DEV)
    rc = _hip.lib().dsp_gnb_fit(_hip.ptr(Xd), _hip.ptr(yd), N, D, C, var_smoothing, _hip.ptr(theta), _hip.ptr(var),
                                _hip.ptr(count), _hip.ptr(eps), _hip.ptr(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    return rc, theta.cpu().numpy(), var.cpu().numpy(), count.cpu().numpy(), float(eps.item())


def labels_for(rng, N, C):
    """Interleaved labels, every class present; class 1 has a single row; when there is room the last
    class's only row is the last one."""
    if N == C:
        return rng.permutation(C)
    keep = [c for c in range(C) if c not in (1, C - 1)] or [0]
    y = np.concatenate([np.arange(C - 1), rng.choice(keep, N - C)])
    rng.shuffle(y)
    return np.concatenate([y, [C - 1]])


@pytest.mark.parametrize("N,D,C", [(2, 2, 2), (10, 15, 10), (64, 17, 64), (257, 2, 10), (257, 40, 2), (513, 15, 64),
                                   (513, 17, 2), (3001, 15, 10), (3001, 40, 64), (3001, 17, 10)])
def test_fit_equals_sklearn_bit_for_bit(N, D, C):
    from sklearn.naive_bayes import GaussianNB
    rng = np.random.default_rng(1000 * N + 10 * D + C)
    y = labels_for(rng, N, C)
    X = rng.normal(0.0, 1.0, (N, D)) * rng.uniform(0.1, 10.0, D) + rng.normal(0.0, 3.0, D)
    m = GaussianNB().fit(X, y)
    rc, theta, var, count, eps = abi_fit(X, y, C)
    assert rc == 0
    assert np.array_equal(theta, m.theta_) and np.array_equal(var, m.var_) and eps == m.epsilon_
    assert np.array_equal(count.astype(np.float64), m.class_count_)
    assert np.array_equal(count / count.sum(), m.class_prior_)
    if N > C:
        assert count[1] == 1 and np.array_equal(var[1], np.full(D, eps))  # a single row: variance = epsilon
        assert count[C - 1] == 1 and np.array_equal(theta[C - 1], X[-1])  # its only row is the last one


def test_fit_refuses_one_column():
    from src import _hip
    rc = abi_fit(np.zeros((10, 1)), np.arange(10) % 2, 2)[0]
    assert rc == _hip.DSP_ERR_ARGS


# ---- dsp_gnb_predict -----------------------------------------------------------------------------
def abi_nb_predict(m, X, with_jll=True):
    """dsp_gnb_predict through the C ABI: (pred, jll, certified, uncertified count)."""
    from src import _hip
    L = _hip.lib()
    X = np.ascontiguousarray(X, dtype=np.float64)
    C, D = m["theta"].shape
    Nq = X.shape[0]
    lp, nc = R.gnb_constants(m)
    nbytes = L.dsp_gnb_workspace_bytes(Nq, D, C)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    th, va, lpd, ncd = (_dev(a, torch.float64) for a in (m["theta"], m["var"], lp, nc))
    q = _dev(X, torch.float64)
    pred = torch.full((Nq,), -1, dtype=torch.int32, device=DEV)
    cert = torch.full((Nq,), -1, dtype=torch.int32, device=DEV)
    jll = torch.full((Nq, C), float("nan"), dtype=torch.float64, device=DEV) if with_jll else None
    rc = L.dsp_gnb_predict(_hip.ptr(th), _hip.ptr(va), _hip.ptr(lpd), _hip.ptr(ncd), D, C, _hip.ptr(q), Nq,
                           _hip.ptr(pred), _hip.ptr(jll), _hip.ptr(cert), _hip.ptr(ws), nbytes, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return (pred.cpu().numpy(), jll.cpu().numpy() if with_jll else None, cert.cpu().numpy(),
            int(ws[:4].view(torch.int32).item()))


def check_nb(m, X, want_pred, want_jll):
    """pred exact, jll within the derived bound, every row certified."""
    pred, jll, cert, unc = abi_nb_predict(m, X)
    bound = R.gnb_bound(m, X)
    err = np.abs(jll - want_jll)
    print("max err / bound %.3g, min margin / threshold %.3g" % ((err / bound).max(), R.gnb_margin_ratio(jll, bound).min()))
    assert np.array_equal(m["classes"][pred], want_pred)
    assert np.all(err <= bound), (err / bound).max()
    assert unc == 0 and np.all(cert == 1)
    return pred, jll


@pytest.mark.parametrize("name", MODELS)
def test_nb_golden_models_c_abi(golden, name):
    m = nb_of(golden, name)
    check_nb(m, golden[name + "/X"], golden[name + "/nb_pred"], golden[name + "/nb_jll"])
    # without the jll output: the same labels and certificates
    pred, _, cert, unc = abi_nb_predict(m, golden[name + "/X"], with_jll=False)
    assert np.array_equal(m["classes"][pred], golden[name + "/nb_pred"]) and unc == 0 and np.all(cert == 1)


@pytest.mark.parametrize("name", MODELS)
def test_nb_near_ties_alone_are_uncertified(golden, name):
    m = nb_of(golden, name)
    T = golden[name + "/tie_X"]
    pred, jll, cert, unc = abi_nb_predict(m, T)
    assert np.all(cert == 0) and unc == 2
    assert np.all(np.abs(jll - golden[name + "/tie_jll"]) <= R.gnb_bound(m, T))
    X = np.concatenate([golden[name + "/X"][:40], T, golden[name + "/X"][40:60]])
    pred, jll, cert, unc = abi_nb_predict(m, X)
    assert unc == 2 and np.flatnonzero(cert == 0).tolist() == [40, 41]


@pytest.mark.parametrize("name", MODELS)
def test_nb_batch_sizes_and_row_bits(golden, name):
    """Nq = 1, 63, 65, 1000 (the golden queries repeated): scikit-learn's labels, and a row's jll bits
    are the same alone, inside every batch and at another position; a repeated launch is bitwise equal."""
    m = nb_of(golden, name)
    X, want, wj = golden[name + "/X"], golden[name + "/nb_pred"], golden[name + "/nb_jll"]
    reps = -(-1000 // len(X))
    X, want, wj = np.tile(X, (reps, 1))[:1000], np.tile(want, reps)[:1000], np.tile(wj, (reps, 1))[:1000]
    first = None
    for n in (1, 63, 65, 1000):
        pred, jll = check_nb(m, X[:n], want[:n], wj[:n])
        if first is None:
            first = jll[0].copy()
        assert np.array_equal(jll[0].view(np.uint64), first.view(np.uint64)), n
    assert np.array_equal(jll[len(golden[name + "/X"])].view(np.uint64), first.view(np.uint64))  # the same row again
    again = abi_nb_predict(m, X)
    assert np.array_equal(again[0], pred) and np.array_equal(again[1].view(np.uint64), jll.view(np.uint64))


def test_nb_bad_rows_are_uncertified(golden):
    m = nb_of(golden, "c10")
    X = golden["c10/X"][:70].copy()
    X[5, 3], X[66, 0] = np.nan, np.inf
    pred, jll, cert, unc = abi_nb_predict(m, X)
    assert unc == 2 and np.flatnonzero(cert == 0).tolist() == [5, 66]
    keep = np.setdiff1d(np.arange(70), [5, 66])
    assert np.array_equal(m["classes"][pred[keep]], golden["c10/nb_pred"][:70][keep])


@pytest.mark.parametrize("C,D", [(1, 5), (5, 1), (64, 33), (7, 130), (3, 2500)])
def test_nb_shapes_fitted_here(C, D):
    """One class, one column, the limits of the class count, columns read from memory (D > 32), a
    stage of several classes with a remainder (D = 130) and a class in two LDS chunks (D = 2500)."""
    from sklearn.naive_bayes import GaussianNB
    rng = np.random.default_rng(100 * C + D)
    centres = rng.normal(0.0, 3.0 / np.sqrt(D), (C, D))
    lab = np.concatenate([np.arange(C), rng.integers(0, C, 6 * C)])
    X = centres[lab] + rng.normal(0.0, 1.0, (len(lab), D))
    nb = GaussianNB().fit(X, lab)
    m = {"theta": nb.theta_, "var": nb.var_, "class_prior": nb.class_prior_, "classes": nb.classes_}
    Q = centres[rng.integers(0, C, 150)] + rng.normal(0.0, 1.0, (150, D))
    ratio = R.gnb_margin_ratio(R.gnb_jll(m, Q), R.gnb_bound(m, Q))
    Q = Q[ratio >= 16.0]  # (a random row on the edge of the certificate would be no failure)
    assert len(Q) >= 140
    check_nb(m, Q, nb.predict(Q), nb._joint_log_likelihood(Q))


# ---- dsp_tree_predict ----------------------------------------------------------------------------
def abi_tree_predict(t, X, with_leaf=True, max_depth=None):
    """dsp_tree_predict through the C ABI: (pred, leaf, unanswered count)."""
    from src import _hip
    L = _hip.lib()
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, (Nq, D) = len(t["left"]), X.shape
    nbytes = L.dsp_tree_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    arrs = [_dev(t[k], torch.int32) for k in ("left", "right", "feature")]
    thr, lc, q = _dev(t["threshold"], torch.float64), _dev(t["leaf_class"], torch.int32), _dev(X, torch.float64)
    pred = torch.full((Nq,), -7, dtype=torch.int32, device=DEV)
    leaf = torch.full((Nq,), -7, dtype=torch.int32, device=DEV) if with_leaf else None
    depth = int(t["max_depth"]) if max_depth is None else max_depth
    rc = L.dsp_tree_predict(_hip.ptr(arrs[0]), _hip.ptr(arrs[1]), _hip.ptr(arrs[2]), _hip.ptr(thr), _hip.ptr(lc), n,
                            depth, D, _hip.ptr(q), Nq, _hip.ptr(pred), _hip.ptr(leaf), _hip.ptr(ws), nbytes, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return pred.cpu().numpy(), leaf.cpu().numpy() if with_leaf else None, int(ws[:4].view(torch.int32).item())


@pytest.mark.parametrize("name", MODELS + ("one",))
def test_tree_golden_c_abi(golden, name):
    t = tree_of(golden, name)
    pred, leaf, bad = abi_tree_predict(t, golden[name + "/X"])
    assert bad == 0 and np.array_equal(leaf, golden[name + "/tree_apply"])
    assert np.array_equal(t["classes"][pred], golden[name + "/tree_pred"])
    assert np.array_equal(abi_tree_predict(t, golden[name + "/X"], with_leaf=False)[0], pred)
    if name != "one":  # at, one float32 ulp above and below the threshold, and the row the cast decides
        pred, leaf, bad = abi_tree_predict(t, golden[name + "/bnd_X"])
        assert bad == 0 and np.array_equal(leaf, golden[name + "/bnd_apply"])
        assert np.array_equal(t["classes"][pred], golden[name + "/bnd_pred"])


@pytest.fixture(scope="module")
def deep_tree():
    """20 000 noisy rows: more nodes than the LDS-resident table holds, depth over 30."""
    from sklearn.tree import DecisionTreeClassifier
    rng = np.random.default_rng(21)
    X = rng.normal(0.0, 1.0, (20000, 5))
    y = (X[:, 0] + 0.6 * rng.normal(0.0, 1.0, 20000) > 0).astype(np.int64) + 2 * (rng.random(20000) < 0.08)
    tree = DecisionTreeClassifier(random_state=42).fit(X, y)
    return tree, rng.normal(0.0, 1.0, (3000, 5))


def test_tree_deep_and_beyond_lds(deep_tree):
    from src import _hip
    tree, Q = deep_tree
    t = R.tree_arrays(tree)
    assert len(t["left"]) > 4000 and tree.tree_.max_depth > 30, (len(t["left"]), tree.tree_.max_depth)
    assert len(t["left"]) > _hip.lib().dsp_tree_lds_nodes()  # the table is read from memory
    pred, leaf, bad = abi_tree_predict(t, Q)
    assert bad == 0 and np.array_equal(leaf, tree.apply(Q)) and np.array_equal(t["classes"][pred], tree.predict(Q))
    # a walk cut short by max_depth ends with -1 instead of going on
    deep = np.asarray(tree.decision_path(Q).sum(axis=1)).ravel() - 1 > 10
    pred, leaf, bad = abi_tree_predict(t, Q, max_depth=10)
    assert np.array_equal(leaf < 0, deep) and bad == int(deep.sum()) and np.array_equal(pred < 0, deep)
    assert np.array_equal(leaf[~deep], tree.apply(Q)[~deep])


def test_tree_lds_resident_is_the_same_walk(deep_tree):
    """A tree cut at depth 22: a table of some 2 000 nodes that fits LDS, also against the restatement."""
    from sklearn.tree import DecisionTreeClassifier
    from src import _hip
    rng = np.random.default_rng(22)
    X = rng.normal(0.0, 1.0, (6000, 5))
    y = rng.integers(0, 3, 6000)
    tree = DecisionTreeClassifier(max_depth=22, random_state=42).fit(X, y)
    t = R.tree_arrays(tree)
    assert 1000 < len(t["left"]) <= _hip.lib().dsp_tree_lds_nodes()
    Q = deep_tree[1]
    pred, leaf, bad = abi_tree_predict(t, Q)
    assert bad == 0 and np.array_equal(leaf, tree.apply(Q)) and np.array_equal(leaf, R.tree_walk(t, Q)[1])


def test_tree_bad_rows_and_malformed_tables(golden):
    t = tree_of(golden, "c10")
    X = golden["c10/X"][:300].copy()
    X[7, 2], X[258, 14], X[299, 0] = np.nan, 3.5e38, -np.inf  # 3.5e38 is finite, but not as float32
    pred, leaf, bad = abi_tree_predict(t, X)
    assert bad == 3 and np.flatnonzero(leaf < 0).tolist() == [7, 258, 299] and np.all(pred[[7, 258, 299]] == -1)
    keep = leaf >= 0
    assert np.array_equal(leaf[keep], golden["c10/tree_apply"][:300][keep])
    # hand-made tables: a child pointing backwards, at itself, past the end; a feature past D
    base = {"left": np.array([1, -1, 3, -1, -1], np.int32), "right": np.array([2, -1, 4, -1, -1], np.int32),
            "feature": np.array([0, -2, 1, -2, -2], np.int32), "threshold": np.array([0.0, -2.0, 0.0, -2.0, -2.0]),
            "leaf_class": np.array([0, 0, 0, 1, 2], np.int32), "max_depth": 2}
    Q = np.array([[-1.0, 0.0], [1.0, -1.0], [1.0, 1.0]])
    pred, leaf, bad = abi_tree_predict(base, Q)
    assert leaf.tolist() == [1, 3, 4] and pred.tolist() == [0, 1, 2] and bad == 0
    for key, node, value, want in (("right", 2, 0, [1, 3, -1]), ("left", 2, 2, [1, -1, 4]), ("right", 0, 5, [1, -1, -1]),
                                   ("left", 0, -3, [-1, 3, 4]), ("feature", 2, 2, [1, -1, -1])):
        bad_t = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        bad_t[key][node] = value
        pred, leaf, bad = abi_tree_predict(bad_t, Q, max_depth=1000)
        assert leaf.tolist() == want and bad == want.count(-1), (key, leaf)
        assert np.array_equal(leaf, R.tree_walk(dict(bad_t, max_depth=1000), Q)[1])


# ---- Python surface --------------------------------------------------------------------------------
def test_index_surface(golden):
    from src.pipeline import GnbIndex, TreeIndex
    nb, tree, Q = sk_models("c3")
    idx = GnbIndex(nb)
    stats = {}
    pred, jll, cert = idx.query(golden["c3/X"], with_jll=True, stats=stats)
    assert stats == {"uncertified": 0} and pred.is_cuda and jll.shape == (300, 3) and cert.dtype == torch.int32
    assert np.array_equal(golden["c3/classes"][pred.cpu().numpy()], golden["c3/nb_pred"])
    pred, jll, cert = idx.query(np.empty((0, 40)), stats=stats)
    assert pred.shape == (0,) and jll is None and stats == {"uncertified": 0}
    with pytest.raises(ValueError):
        idx.query(np.zeros((3, 39)))
    tidx = TreeIndex(tree)
    pred, leaf = tidx.query(torch.as_tensor(golden["c3/X"], device=DEV), stats=stats)
    assert stats["unanswered"] == 0 and leaf.is_cuda and leaf.dtype == torch.int32
    assert np.array_equal(leaf.cpu().numpy(), golden["c3/tree_apply"])
    with pytest.raises(ValueError):
        tidx.query(np.zeros((3, 41)))


@pytest.mark.parametrize("name", MODELS)
def test_classifier_predicts_like_sklearn(golden, name):
    """TraditionalClassifier for both types on ordinary plus special rows."""
    from src.models import TraditionalClassifier
    nb, tree, _ = sk_models(name)
    assert np.array_equal(nb.theta_, golden[name + "/theta"])
    clf = TraditionalClassifier('naive_bayes')
    clf.model = nb
    X = np.concatenate([golden[name + "/X"], golden[name + "/tie_X"]])
    got = clf.predict(X)
    assert np.array_equal(got, np.concatenate([golden[name + "/nb_pred"], golden[name + "/tie_pred"]]))
    assert np.array_equal(got, nb.predict(X)) and clf.last_predict_stats == {'device': True, 'uncertified': 2}
    assert np.array_equal(clf.predict(golden[name + "/X"]), golden[name + "/nb_pred"])
    assert clf.last_predict_stats == {'device': True, 'uncertified': 0}

    clf = TraditionalClassifier('decision_tree')
    clf.model = tree
    X = np.concatenate([golden[name + "/X"], golden[name + "/bnd_X"]])
    got = clf.predict(X)
    assert np.array_equal(got, np.concatenate([golden[name + "/tree_pred"], golden[name + "/bnd_pred"]]))
    assert np.array_equal(got, tree.predict(X)) and clf.last_predict_stats == {'device': True, 'uncertified': 0}
    leaves = clf.apply(X)
    assert leaves.dtype == np.int64 and np.array_equal(leaves, tree.apply(X))
    # rows the device leaves unanswered are scikit-learn's: its answer for a NaN (a missing value goes
    # to the larger child), its own error for a value that is not finite as float32
    X[3, 0] = np.nan
    assert np.array_equal(clf.predict(X), tree.predict(X)) and np.array_equal(clf.apply(X), tree.apply(X))
    assert clf.last_predict_stats == {'device': True, 'uncertified': 1}
    X[5, 1] = 1e39
    with pytest.raises(ValueError):
        clf.predict(X)
    assert clf.last_predict_stats == {'device': True, 'uncertified': 2}


def test_a_query_cut_into_two_launches(golden, monkeypatch):
    """(dsp_gnb_predict's row count is its argument 7.)"""
    from src.pipeline import GnbIndex
    cases.check_two_launches(monkeypatch, GnbIndex, "dsp_gnb_predict", 7, sk_models("c3")[0], golden["c3/X"],
                             golden["c3/tie_X"], with_jll=True)


@pytest.mark.parametrize("name", MODELS)
def test_classifier_takes_device_rows(golden, name):
    """Ordinary rows plus the special ones (the two near ties; for the tree a NaN), as host rows and as a
    float64 device tensor."""
    from src.models import TraditionalClassifier
    nb, tree, _ = sk_models(name)
    clf = TraditionalClassifier('naive_bayes')
    clf.model = nb
    cases.check_device_rows(clf, np.concatenate([golden[name + "/X"], golden[name + "/tie_X"]]), 2)
    clf = TraditionalClassifier('decision_tree')
    clf.model = tree
    X = golden[name + "/X"].copy()
    X[3, 0] = np.nan
    cases.check_device_rows(clf, X, 1)


def _blobs():
    rng = np.random.default_rng(4)
    centres = rng.normal(0.0, 1.0, (4, 15))
    lab = rng.integers(0, 4, 1400)
    X = centres[lab] + rng.normal(0.0, 1.0, (1400, 15))
    return X[:1000], lab[:1000] * 2 + 1, X[1000:], lab[1000:] * 2 + 1


@pytest.mark.parametrize("kind", ["svm", "naive_bayes", "decision_tree"])
def test_upload_follows_the_fitted_model(kind):
    """One contract for the three scikit-learn-backed types: the upload is kept between predicts, made
    again after a refit on the model itself, dropped by ``fit``; the labels are the model's own."""
    from src.models import create_classifier
    Xtr, ytr, Xte, _ = _blobs()
    clf = create_classifier(kind).fit(Xtr, ytr)
    assert clf._index is None
    assert np.array_equal(clf.predict(Xte), clf.model.predict(Xte)) and clf.last_predict_stats['device'] is True
    first = clf._index
    assert np.array_equal(clf.predict(Xte[:10]), clf.model.predict(Xte[:10])) and clf._index is first
    clf.model.fit(Xtr[:, :7], ytr)  # a refit made on the model directly: the upload follows the model
    assert np.array_equal(clf.predict(Xte[:, :7]), clf.model.predict(Xte[:, :7])) and clf._index is not first
    assert clf.last_predict_stats['device'] is True
    clf.fit(Xtr, ytr)
    assert clf._index is None
    assert np.array_equal(clf.predict(Xte), clf.model.predict(Xte)) and clf.last_predict_stats['device'] is True


def test_refit_uploads_again_and_device_fit_completes_the_model():
    """(The refit half is test_upload_follows_the_fitted_model.)"""
    from sklearn.naive_bayes import GaussianNB
    from src.models import create_classifier
    Xtr, ytr, Xte, yte = _blobs()
    # fit on device rows: .model is a complete GaussianNB with scikit-learn's own bits
    clf = create_classifier('naive_bayes').fit(torch.as_tensor(Xtr, device=DEV), ytr)
    want = GaussianNB().fit(Xtr, ytr)
    for attr in ("classes_", "class_count_", "class_prior_", "theta_", "var_"):
        assert np.array_equal(getattr(clf.model, attr), getattr(want, attr)), attr
    assert clf.model.epsilon_ == want.epsilon_ and clf.model.n_features_in_ == 15
    assert np.array_equal(clf.model.predict(Xte), want.predict(Xte))
    assert np.array_equal(clf.predict(torch.as_tensor(Xte, device=DEV)), want.predict(Xte))
    res = clf.evaluate(Xte, yte)
    assert np.array_equal(res['predictions'], want.predict(Xte))


def test_classifier_comparison_reports_sklearns_accuracies(tmp_path):
    from sklearn.metrics import accuracy_score
    from sklearn.naive_bayes import GaussianNB
    from sklearn.tree import DecisionTreeClassifier
    from experiments.run_experiments import SpeechRecognitionExperiment
    rng = np.random.default_rng(12)
    centres = rng.normal(0.0, 0.9, (5, 15))
    lab = rng.integers(0, 5, 600)
    exp = SpeechRecognitionExperiment(str(tmp_path / "none"), str(tmp_path / "res"))
    exp.X, exp.y = centres[lab] + rng.normal(0.0, 1.0, (600, 15)), lab
    exp.class_names = ["w%d" % c for c in range(5)]
    res = exp.experiment_classifier_comparison(classifiers={'Naive Bayes': ('naive_bayes', {}),
                                                            'Decision Tree': ('decision_tree', {})})
    Xtr, Xte, ytr, yte = exp.split_normalize()
    for name, model in (('Naive Bayes', GaussianNB()), ('Decision Tree', DecisionTreeClassifier(max_depth=None, random_state=42))):
        want = model.fit(Xtr, ytr).predict(Xte)
        assert np.array_equal(res[name]['predictions'], want) and res[name]['accuracy'] == accuracy_score(yte, want)
