"""CPU checks of the SVC prediction feature: the numpy restatement of libsvm's predict
(tests/svc_reference.py) against the golden scikit-learn results, the derived bound, the new
exports, the golden file's reproducibility, and the scikit-learn path of the other kernels."""
import ctypes
import os
import sys

import numpy as np
import pytest

import svc_reference as R
from conftest import GOLDEN

MODELS = ("c2", "c3", "c10")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "svc_golden.npz"))


def model_of(g, name):
    return {k: g["%s/%s" % (name, k)] for k in ("sv", "n_support", "dual_coef", "intercept", "gamma", "classes")}


def test_golden_covers_the_planned_models(golden):
    m = {n: model_of(golden, n) for n in MODELS}
    assert [len(m[n]["classes"]) for n in MODELS] == [2, 3, 10]
    assert 40 <= m["c2"]["sv"].shape[0] <= 90 and 1000 <= m["c10"]["sv"].shape[0] <= 1200
    assert m["c3"]["classes"].tolist() == [3, 7, 11]
    for n in MODELS:
        assert m[n]["sv"].shape[1] == 15 and 64 <= golden[n + "/X"].shape[0] <= 600
        assert golden[n + "/tie_X"].shape == (2, 15)
        assert int(m[n]["n_support"].sum()) == m[n]["sv"].shape[0]


@pytest.mark.parametrize("name", MODELS)
def test_restatement_predicts_like_sklearn(golden, name):
    m = model_of(golden, name)
    assert np.array_equal(R.predict(m, golden[name + "/X"]), golden[name + "/pred"])


@pytest.mark.parametrize("name", MODELS)
def test_restatement_dec_within_the_derived_bound(golden, name):
    """Two fp64 evaluations of the contract (numpy's and libsvm's) differ by at most the bound --
    near-tie queries included -- and the ordinary queries are decided with room to spare: the
    smallest |dec| is more than 1e6 times the bound, so all of them certify."""
    m = model_of(golden, name)
    for X, want in ((golden[name + "/X"], golden[name + "/dec"]), (golden[name + "/tie_X"], golden[name + "/tie_dec"])):
        dec = R.decision_values(m, X)
        bound = R.dec_bound(m, X)
        err = np.abs(R.sklearn_signs(dec) - want).reshape(dec.shape)
        assert np.all(err <= bound), (err.max(), bound.min())
    dec, bound = R.decision_values(m, golden[name + "/X"]), R.dec_bound(m, golden[name + "/X"])
    assert np.min(np.abs(dec) / bound) > 1e6
    tie = R.decision_values(m, golden[name + "/tie_X"])
    assert np.all(np.abs(tie[:, 0]) < R.dec_bound(m, golden[name + "/tie_X"])[:, 0])  # uncertifiable


def test_exports_are_typed_and_abi_is_6():
    from src import _hip
    lib = _hip.load_library()
    assert lib.dsp_abi_version() == 6 and _hip.ABI_VERSION == 6
    for name in ("dsp_svc_workspace_bytes", "dsp_svc_workspace_uncertified_offset", "dsp_svc_launch_parts",
                 "dsp_svc_predict"):
        assert name in _hip.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.dsp_svc_predict.argtypes[7] is ctypes.c_double  # gamma
    # sizes: outside the plan 0, inside > 0 with the counter inside the workspace
    w = lib.dsp_svc_workspace_bytes
    assert w(1000, 100, 15, 10) > 0 and w(1000, 100, 4096, 64) > 0
    assert w(1000, 100, 0, 10) == 0 and w(1000, 100, 4097, 10) == 0
    assert w(1000, 100, 15, 1) == 0 and w(1000, 100, 15, 65) == 0 and w(0, 100, 15, 10) == 0
    assert 0 < lib.dsp_svc_workspace_uncertified_offset(1000, 100, 15, 10) + 4 <= w(1000, 100, 15, 10)
    # few queries against many support vectors split the support vectors; many queries do not;
    # a model of one segment has nothing to split
    parts = lib.dsp_svc_launch_parts
    assert parts(1109, 65, 15, 10) > 1 and parts(1109, 600, 15, 10) == 1 and parts(65, 5, 15, 2) == 1
    # host argument checks come before any launch
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.dsp_svc_predict
    assert f(p, p, p, p, 10, 15, 1, 0.1, p, 4, p, None, p, p, 1 << 20, None) == _hip.DSP_ERR_ARGS
    assert f(p, p, p, p, 10, 15, 3, -1.0, p, 4, p, None, p, p, 1 << 20, None) == _hip.DSP_ERR_ARGS
    assert f(p, p, p, p, 10, 15, 3, 0.1, p, 4, p, None, p, None, 0, None) == _hip.DSP_ERR_WORKSPACE
    assert f(p, p, p, p, 10, 15, 3, 0.1, None, 0, None, None, None, None, 0, None) == _hip.DSP_OK


def test_make_svc_golden_reproduces_the_committed_predictions(golden):
    sys.path.insert(0, GOLDEN)
    try:
        import make_svc_golden
    finally:
        sys.path.remove(GOLDEN)
    fresh = make_svc_golden.build()
    for name in MODELS:
        assert np.array_equal(fresh[name + "/X"], golden[name + "/X"])
        assert np.array_equal(fresh[name + "/pred"], golden[name + "/pred"])
        assert np.array_equal(fresh[name + "/n_support"], golden[name + "/n_support"])


def test_linear_kernel_still_predicts_through_sklearn():
    """No device is touched: a linear SVC is outside the kernel's plan, so predict is the model's."""
    from src.models import TraditionalClassifier
    rng = np.random.default_rng(5)
    X = np.concatenate([rng.normal(-1, 1, (40, 4)), rng.normal(1, 1, (40, 4))])
    y = np.repeat([2, 9], 40)
    clf = TraditionalClassifier('svm', kernel='linear').fit(X, y)
    assert np.array_equal(clf.predict(X), clf.model.predict(X))
    assert clf.last_predict_stats == {'device': False, 'uncertified': 0}
    assert np.array_equal(clf.decision_function(X), clf.model.decision_function(X))


def test_in_plan_decides_on_the_host(monkeypatch):
    """SvcIndex.in_plan asks no device: the ordinary fitted model is inside the plan; sparse rows, a model
    fitted on sparse rows, a linear kernel and an unfitted model are outside it, and predict then is
    scikit-learn's with the "off" record."""
    import torch
    from scipy.sparse import csr_matrix
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from src.models import TraditionalClassifier
    from src.pipeline import SvcIndex
    rng = np.random.default_rng(7)
    X = np.concatenate([rng.normal(-1, 1, (40, 4)), rng.normal(1, 1, (40, 4))])
    y = np.repeat([2, 9], 40)
    off = {'device': False, 'uncertified': 0}
    clf = TraditionalClassifier('svm')
    assert not SvcIndex.in_plan(clf.model, X)  # not fitted
    clf.fit(X, y)
    assert SvcIndex.in_plan(clf.model, X) and not SvcIndex.in_plan(clf.model, csr_matrix(X))
    sparse = TraditionalClassifier('svm').fit(csr_matrix(X), y)
    assert not SvcIndex.in_plan(sparse.model, csr_matrix(X)) and not SvcIndex.in_plan(sparse.model, X)
    for rows in (csr_matrix(X), X):
        sparse.last_predict_stats = None
        assert np.array_equal(sparse.predict(rows), sparse.model.predict(rows)) and sparse.last_predict_stats == off
    linear = TraditionalClassifier('svm', kernel='linear').fit(X, y)
    assert not SvcIndex.in_plan(linear.model, X)
    linear.last_predict_stats = None
    assert np.array_equal(linear.predict(X), linear.model.predict(X)) and linear.last_predict_stats == off


def test_rbf_predict_needs_the_device(monkeypatch):
    """Like every accelerated entry point: no quiet fall-back to the host."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from src import _hip
    from src.models import TraditionalClassifier
    rng = np.random.default_rng(6)
    X = np.concatenate([rng.normal(-1, 1, (30, 3)), rng.normal(1, 1, (30, 3))])
    clf = TraditionalClassifier('svm').fit(X, np.repeat([0, 1], 30))
    with pytest.raises(_hip.HipError):
        clf.predict(X)
