"""SVC prediction on the MI355X (csrc/svm.hip, dsp_svc_predict) against scikit-learn: the golden
models (tests/golden/svc_golden.npz), the near-tie queries and their fallback, the launch shapes,
and the Python surface (SvcIndex, TraditionalClassifier('svm')).

The tolerance on dec is the derived bound of tests/svc_reference.dec_bound,
computed on the CPU from the model and the queries."""
import os

import numpy as np
import pytest
import torch

import predict_path_cases as cases
import svc_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODELS = ("c2", "c3", "c10")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "svc_golden.npz"))


def model_of(g, name):
    return {k: g["%s/%s" % (name, k)] for k in ("sv", "n_support", "dual_coef", "intercept", "gamma", "classes")}


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def abi_predict(m, X):
    """dsp_svc_predict through the C ABI: (pred, dec [Nq, P] libsvm signs, certified, uncertified count)."""
    from src import _hip
    L = _hip.lib()
    X = np.ascontiguousarray(X, dtype=np.float64)
    nSV, D = m["sv"].shape
    C, Nq = len(m["n_support"]), X.shape[0]
    P = C * (C - 1) // 2
    nbytes = L.dsp_svc_workspace_bytes(nSV, Nq, D, C)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    sv, ns = _dev(m["sv"], torch.float64), _dev(m["n_support"], torch.int32)
    coef, b, q = _dev(m["dual_coef"], torch.float64), _dev(m["intercept"], torch.float64), _dev(X, torch.float64)
    pred = torch.full((Nq,), -1, dtype=torch.int32, device=DEV)
    cert = torch.full((Nq,), -1, dtype=torch.int32, device=DEV)
    dec = torch.full((Nq, P), float("nan"), dtype=torch.float64, device=DEV)
    rc = L.dsp_svc_predict(_hip.ptr(sv), _hip.ptr(ns), _hip.ptr(coef), _hip.ptr(b), nSV, D, C, float(m["gamma"]),
                           _hip.ptr(q), Nq, _hip.ptr(pred), _hip.ptr(dec), _hip.ptr(cert), _hip.ptr(ws), nbytes,
                           _hip.stream_handle(torch.device(DEV)))
    assert rc == 0, rc
    torch.cuda.synchronize()
    off = L.dsp_svc_workspace_uncertified_offset(nSV, Nq, D, C)
    return (pred.cpu().numpy(), dec.cpu().numpy(), cert.cpu().numpy(),
            int(ws[off:off + 4].view(torch.int32).item()))


def check_against(m, X, want_pred, want_dec_sklearn):
    """pred exact, dec within the derived bound, every row certified."""
    pred, dec, cert, unc = abi_predict(m, X)
    bound = R.dec_bound(m, X)
    err = np.abs(R.sklearn_signs(dec) - want_dec_sklearn).reshape(dec.shape)
    print("max err / bound %.3g, min |dec| / bound %.3g" % ((err / bound).max(), (np.abs(dec) / bound).min()))
    assert np.array_equal(m["classes"][pred], want_pred)
    assert np.all(err <= bound), (err / bound).max()
    assert unc == 0 and np.all(cert == 1)
    return pred, dec


@pytest.mark.parametrize("name", MODELS)
def test_golden_models_c_abi(golden, name):
    m = model_of(golden, name)
    check_against(m, golden[name + "/X"], golden[name + "/pred"], golden[name + "/dec"])


@pytest.mark.parametrize("name", MODELS)
def test_near_ties_are_uncertified(golden, name):
    """|dec_0| of the bisected queries is 1e-16 .. 1e-15: no rounding bound can decide them; dec itself
    is still within the bound of scikit-learn's."""
    m = model_of(golden, name)
    T = golden[name + "/tie_X"]
    pred, dec, cert, unc = abi_predict(m, T)
    assert np.all(cert == 0) and unc == 2
    err = np.abs(R.sklearn_signs(dec) - golden[name + "/tie_dec"]).reshape(dec.shape)
    assert np.all(err <= R.dec_bound(m, T))
    # mixed with ordinary queries: only the two near ties lose their certificate
    X = np.concatenate([golden[name + "/X"][:40], T, golden[name + "/X"][40:60]])
    pred, dec, cert, unc = abi_predict(m, X)
    assert unc == 2 and np.flatnonzero(cert == 0).tolist() == [40, 41]


def sk_model(golden, name):
    """The scikit-learn model the golden file was made from, refitted (tests/golden/make_svc_golden.py)."""
    import sys
    sys.path.insert(0, GOLDEN)
    try:
        import make_svc_golden
    finally:
        sys.path.remove(GOLDEN)
    m, _ = make_svc_golden.fit(name)
    return m


@pytest.mark.parametrize("name", MODELS)
def test_classifier_answers_near_ties_with_sklearn(golden, name):
    """TraditionalClassifier.predict on ordinary + near-tie rows: sklearn's labels, two rows redone."""
    from src.models import TraditionalClassifier
    clf = TraditionalClassifier('svm', C=1.0, kernel='rbf')
    clf.model = sk_model(golden, name)  # the model the golden file was made from
    assert np.array_equal(clf.model.support_vectors_, golden[name + "/sv"])
    X = np.concatenate([golden[name + "/X"], golden[name + "/tie_X"]])
    want = np.concatenate([golden[name + "/pred"], golden[name + "/tie_pred"]])
    got = clf.predict(X)
    assert np.array_equal(got, want) and np.array_equal(got, clf.model.predict(X))
    assert clf.last_predict_stats == {'device': True, 'uncertified': 2}
    dec = clf.decision_function(golden[name + "/X"])
    assert dec.shape == golden[name + "/dec"].shape
    bound = R.dec_bound(model_of(golden, name), golden[name + "/X"])
    assert np.all(np.abs(dec - golden[name + "/dec"]).reshape(bound.shape) <= bound)
    assert clf.last_predict_stats == {'device': True, 'uncertified': 0}


def test_launch_shapes_agree_bitwise(golden):
    """Nq = 1, 5, 63, 65, 600 against the C = 10 model: the SV-split launch (few queries) and the
    query-tiled launch both run, every one matches scikit-learn, and the first five queries come back
    with the same bits -- dec included -- from all of them; a repeated launch is bitwise equal."""
    from src import _hip
    m = model_of(golden, "c10")
    X, want, wdec = golden["c10/X"], golden["c10/pred"], golden["c10/dec"]
    nSV, D = m["sv"].shape
    parts = [_hip.lib().dsp_svc_launch_parts(nSV, n, D, 10) for n in (1, 5, 63, 65, 600)]
    assert parts[0] > 1 and parts[-1] == 1, parts
    first = None
    for n in (1, 5, 63, 65, 600):
        pred, dec = check_against(m, X[:n], want[:n], wdec[:n])
        k = min(n, 5)
        if first is None:
            first = (pred[:1], dec[:1])
        if n >= 5 and first[0].shape[0] == 1:
            first = (pred[:5], dec[:5])
        assert np.array_equal(pred[:k], first[0][:k])
        assert np.array_equal(dec[:k].view(np.uint64), first[1][:k].view(np.uint64)), n
    a, b = abi_predict(m, X), abi_predict(m, X)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    assert np.array_equal(a[2], b[2])
    a, b = abi_predict(m, X[:65]), abi_predict(m, X[:65])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))


def fit_sklearn(X, y):
    from sklearn.svm import SVC
    m = SVC(C=1.0, kernel='rbf', random_state=42).fit(X, y)
    m.decision_function_shape = 'ovo'
    return m


def check_fitted(m, Q):
    check_against(R.model_arrays(m), Q, m.predict(Q), m.decision_function(Q))


def test_small_and_multi_tile_classes():
    """One LDS tile is 32 support vectors and a class's rows are walked in ceil(nSV / 256) segments:
    two broad overlapping classes give segments of several tiles with a remainder, and a rare third
    class has fewer support vectors than one tile.  Few and many queries: both launches."""
    rng = np.random.default_rng(11)
    X = np.concatenate([rng.normal(0.0, 1.0, (300, 6)), rng.normal(0.4, 1.0, (300, 6)), rng.normal(4.0, 0.3, (12, 6))])
    y = np.repeat([5, 1, 8], [300, 300, 12])
    m = fit_sklearn(X, y)
    ns = m._n_support
    G = -(-int(ns.sum()) // 256)
    assert ns.min() < 32 and ns.max() // G > 2 * 32 and (ns.max() // G) % 32 != 0, (ns, G)
    Q = np.concatenate([rng.normal(0.2, 1.2, (580, 6)), rng.normal(4.0, 0.5, (20, 6))])
    rng.shuffle(Q)
    check_fitted(m, Q)
    check_fitted(m, Q[:37])


@pytest.mark.parametrize("D", [1, 16, 33, 130])
def test_dimensions(D):
    """D = 1 and 16 (query in 16 registers, no padding at 16), 33 and 130 (chunks of 16 with a
    remainder), fitted at test time; three classes, few and many queries."""
    rng = np.random.default_rng(100 + D)
    centres = rng.normal(0.0, 2.0 / np.sqrt(D), (3, D))
    X = np.concatenate([c + rng.normal(0.0, 1.0, (90, D)) for c in centres])
    y = np.repeat([0, 1, 2], 90)
    m = fit_sklearn(X, y)
    Q = centres[rng.integers(0, 3, 530)] + rng.normal(0.0, 1.0, (530, D))
    check_fitted(m, Q)
    check_fitted(m, Q[:9])


@pytest.mark.parametrize("C,D", [(12, 15), (40, 15), (40, 40), (64, 3)])
def test_many_classes(C, D):
    """More than 10 classes: the kernels with 31 and 63 coefficient rows (C <= 32, C <= 64), with
    the query in registers and in chunks; C = 64 is the plan's limit."""
    rng = np.random.default_rng(1000 * C + D)
    centres = rng.normal(0.0, 1.5, (C, D))
    X = np.concatenate([c + rng.normal(0.0, 1.0, (10, D)) for c in centres])
    y = np.repeat(np.arange(C) * 3 + 1, 10)
    m = fit_sklearn(X, y)
    Q = centres[rng.integers(0, C, 150)] + rng.normal(0.0, 1.0, (150, D))
    check_fitted(m, Q)


def test_svc_index_surface(golden):
    from src.pipeline import SvcIndex
    idx = SvcIndex(sk_model(golden, "c3"))
    stats = {}
    pred, dec, cert = idx.query(golden["c3/X"], with_dec=True, stats=stats)
    assert stats == {"uncertified": 0} and pred.is_cuda and dec.shape == (200, 3) and cert.dtype == torch.int32
    assert np.array_equal(golden["c3/classes"][pred.cpu().numpy()], golden["c3/pred"])
    pred, dec, cert = idx.query(np.empty((0, 15)), stats=stats)
    assert pred.shape == (0,) and dec is None and cert.shape == (0,) and stats == {"uncertified": 0}
    with pytest.raises(ValueError):
        idx.query(np.zeros((3, 14)))


def test_a_query_cut_into_two_launches(golden, monkeypatch):
    """(dsp_svc_predict's row count is its argument 9.)"""
    from src.pipeline import SvcIndex
    cases.check_two_launches(monkeypatch, SvcIndex, "dsp_svc_predict", 9, sk_model(golden, "c10"), golden["c10/X"],
                             golden["c10/tie_X"], with_dec=True)


@pytest.mark.parametrize("name", MODELS)
def test_classifier_takes_device_rows(golden, name):
    """Ordinary rows plus the two near ties, as host rows and as a float64 device tensor."""
    from src.models import TraditionalClassifier
    clf = TraditionalClassifier('svm', C=1.0, kernel='rbf')
    clf.model = sk_model(golden, name)
    cases.check_device_rows(clf, np.concatenate([golden[name + "/X"], golden[name + "/tie_X"]]), 2)


def test_evaluate_equals_sklearn():
    """create_classifier('svm', C=1.0, kernel='rbf').evaluate on 400 x 15 rows: the dictionary
    scikit-learn's own model gives."""
    from sklearn.metrics import accuracy_score, classification_report, confusion_matrix
    from src.models import create_classifier
    rng = np.random.default_rng(3)
    centres = rng.normal(0.0, 1.0, (4, 15))
    lab = rng.integers(0, 4, 1400)
    X = centres[lab] + rng.normal(0.0, 1.0, (1400, 15))
    Xtr, ytr, Xte, yte = X[:1000], lab[:1000], X[1000:], lab[1000:]
    clf = create_classifier('svm', C=1.0, kernel='rbf').fit(Xtr, ytr)
    res = clf.evaluate(Xte, yte)
    assert clf.last_predict_stats['device'] is True
    want = clf.model.predict(Xte)
    assert np.array_equal(res['predictions'], want)
    assert res['accuracy'] == accuracy_score(yte, want)
    assert np.array_equal(res['confusion_matrix'], confusion_matrix(yte, want))
    assert res['classification_report'] == classification_report(yte, want, output_dict=True, zero_division=0)
    # a refit made on the model directly: the upload follows the model
    clf.model.fit(Xtr[:, :7], ytr)
    assert np.array_equal(clf.predict(Xte[:, :7]), clf.model.predict(Xte[:, :7]))
    assert clf.last_predict_stats['device'] is True
