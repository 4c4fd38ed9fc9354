"""CPU checks of the SVC edge cases (tests/svc_edge_cases.py): the exact decimal value of the contract
against the two fp64 evaluations the derived bound is about, every case hitting what it claims, and
the host-only launch plan of csrc/svm.hip read through the loaded library."""
import numpy as np
import pytest

import svc_edge_cases as E
import svc_reference as R

TINY = np.finfo(np.float64).tiny


def hand_models():
    out = [E.class_count_model(C) for C in E.CLASS_COUNTS] + [E.dim_model(D) for D in E.DIMS]
    out += [E.class_count_model(C, D) for C, D in E.CORNERS]
    out += list(E.segment_models().values()) + [E.query_count_model(), E.byte_cap_model()]
    return out


@pytest.mark.parametrize("m", hand_models(), ids=lambda m: m['name'])
def test_exact_value_against_the_restatement(m):
    """|exact - numpy| <= dec_bound: the bound is between two fp64 evaluations, the exact value lies at
    most half of it from each."""
    X = E.queries(m, 12, 7)
    X = X[E.exact_rows(m, 12)]
    err = np.abs(E.exact_dec(m, X)[1] - R.decision_values(m, X))
    bound = R.dec_bound(m, X)
    assert np.all(err <= bound), (err / bound).max()
    assert np.all(err <= 0.5 * bound), (err / bound).max()  # (numpy's side alone has half the bound)


@pytest.mark.parametrize("C,D", [(2, 4), (3, 4), (11, 6)])
def test_exact_value_against_libsvm(C, D):
    sk, m, X = E.fitted(C, D)
    Q = X[::17]
    want = sk._decision_function(Q)
    err = np.abs(R.sklearn_signs(E.exact_dec(m, Q)[1]) - want).reshape(len(Q), -1)
    assert np.all(err <= R.dec_bound(m, Q))


def test_large_model_three_rows():
    m = E.large_model()
    assert m['sv'].shape == (16385, 2) and m['n_support'].tolist() == [1, 16000, 384]
    X = E.queries(m, 600, 8)[[0, 2, 4]]
    err = np.abs(E.exact_dec(m, X)[1] - R.decision_values(m, X))
    assert np.all(err <= R.dec_bound(m, X))


def test_shape_cases_hit_their_edges():
    from src import _hip
    parts = _hip.load_library().dsp_svc_launch_parts
    assert {0, 1, 31, 32, 33} <= set(E.TILE_CLASSES)
    for name in ("tiles", "tiles_hd"):
        m = E.segment_models()[name]
        nSV, D = m['sv'].shape
        assert nSV >= 513 and parts(nSV, 5, D, len(E.TILE_CLASSES)) >= 3  # the one-row class at G >= 3
        assert 300 in m['n_support'].tolist()
    assert E.segment_models()["tiles_hd"]['sv'].shape[1] > 32 and E.segment_models()["tiles"]['sv'].shape[1] <= 16
    assert [E.segment_models()[n]['sv'].shape[0] for n in ("nsv256", "nsv257")] == [256, 257]
    for C in E.CLASS_COUNTS:
        ns = E.class_count_model(C)['n_support']
        assert len(ns) == C and (ns == 1).sum() == 1 and ns.max() == 6
    assert E.dim_model(33)['n_support'].tolist() == [15, 16, 9]
    m = E.query_count_model()
    assert m['sv'].shape[0] == 600 and parts(600, 512, 5, 3) == 3 and parts(600, 513, 5, 3) == 1
    m = E.byte_cap_model()
    assert m['sv'].shape[0] == 1025 and len(m['n_support']) == 64
    assert E.EDGE_NQ > 128 and E.EDGE_NQ % 128 != 0


def test_numeric_cases_hit_their_edges():
    sk, m, _ = E.fitted(3, 4)
    nq = E.numeric_queries(m)
    K = R.kernel_values(m, nq["on_sv"])
    n = m['sv'].shape[0]
    assert K[0, 0] == 1.0 and K[1, n // 2] == 1.0 and K[2, n - 1] == 1.0
    x = float(m['gamma']) * np.sum((nq["subnormal"][0] - m['sv'][0]) ** 2)
    K = R.kernel_values(m, nq["subnormal"])
    assert 708 < x < 745 and 0 < K[0, 0] < TINY
    with np.errstate(over='ignore'):
        for name in ("underflow", "huge"):
            K = R.kernel_values(m, nq[name])
            assert np.all(K == 0.0), name
            assert np.array_equal(R.decision_values(m, nq[name]), np.tile(m['intercept'], (len(nq[name]), 1)))
        # scikit-learn accepts the huge finite rows, and libsvm too gets K = 0: the restatement's labels
        assert np.array_equal(sk.predict(nq["huge"]), R.predict(m, nq["huge"]))
    assert np.all(np.isfinite(nq["huge"]))
    exact = E.exact_dec(m, nq["huge"])[1]
    assert np.array_equal(exact, np.tile(m['intercept'], (6, 1)))


@pytest.mark.parametrize("bad", E.NONFINITE)
def test_scikit_learn_refuses_rows_that_are_not_finite(bad):
    """The defect this file's GPU twin pins: an inf row has d^2 = inf, K = 0 and dec = intercept with a
    bound of a few ulp of it -- the restatement would certify what scikit-learn refuses."""
    sk, m, X = E.fitted(3, 4)
    Q = X[:5].copy()
    Q[2, 1] = bad
    for method in (sk.predict, sk.decision_function):
        with pytest.raises(ValueError):
            method(Q)
    if np.isinf(bad):
        with np.errstate(invalid='ignore'):
            dec, bound = R.decision_values(m, Q[2:3]), R.dec_bound(m, Q[2:3])
        assert np.array_equal(dec[0], m['intercept']) and np.min(np.abs(dec) / (R.SAFETY * bound)) > 1e6


def band_cases():
    """(name, model, pair): a fitted C = 2 model, each pair of a fitted C = 3 model, one pair of a
    C = 11 model (31 coefficient rows)."""
    out = [("c2", E.fitted(2, 4)[1], 0)]
    out += [("c3-p%d" % p, E.fitted(3, 4)[1], p) for p in range(3)]
    out += [("c11-p7", E.fitted(11, 6)[1], 7)]
    return out


@pytest.mark.parametrize("name,m,p", band_cases(), ids=[c[0] for c in band_cases()])
def test_banded_queries_stand_where_they_claim(name, m, p):
    X, ratio = E.banded_queries(m, p)
    print(name, np.round(ratio, 4).tolist())
    assert X.shape == (len(E.BAND_KS), m['sv'].shape[1])
    assert np.all(np.abs(ratio - np.array(E.BAND_KS)) <= 0.05), ratio
    assert (np.abs(ratio) <= E.MUST_NOT + 0.05).sum() == 4 and (np.abs(ratio) >= E.MUST - 0.05).sum() == 4


def test_launch_plan_boundaries():
    """The values svc_layout defines, read through the library."""
    from src import _hip
    lib = _hip.load_library()
    assert lib.dsp_abi_version() == 6 and _hip.ABI_VERSION == 6
    parts, w = lib.dsp_svc_launch_parts, lib.dsp_svc_workspace_bytes
    for Nq in (1, 5, 128, 512, 513, 100000):
        assert parts(256, Nq, 4, 3) == 1
    assert parts(257, 512, 4, 3) == 2 and parts(257, 513, 4, 3) == 1
    for nSV in (16384, 16385, 16641):
        assert parts(nSV, 5, 2, 3) == 64
    assert parts(1025, E.BYTE_CAP_NQ[0], 2, 64) == 5 and parts(1025, E.BYTE_CAP_NQ[1], 2, 64) == 1
    assert w(1000, 100, 0, 10) == 0 and w(1000, 100, 4097, 10) == 0
    assert w(1000, 100, 15, 1) == 0 and w(1000, 100, 15, 65) == 0 and w(0, 100, 15, 10) == 0
    assert w(1000, 100, 4096, 64) > 0 and w(1, 1, 1, 2) > 0
