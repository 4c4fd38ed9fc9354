"""CPU checks of the Naive Bayes and Decision Tree edge cases (tests/nb_tree_edge_cases.py): the exact
decimal value of the contract against the fp64 evaluations the derived bound is about, every case hitting
the kernel form, stage, tile or node count it claims, every banded row standing in its window, every
numeric end's written outcome being the restatement's, the tree restatement against scikit-learn's apply
on subnormal thresholds, and the fit restatement against scikit-learn bit for bit."""
import os

import numpy as np
import pytest

import nb_tree_edge_cases as E
import nb_tree_reference as R
from conftest import GOLDEN

MODELS = ("c2", "c3", "c10")
BAND_TOL = 0.05  # every banded row's exact margin / threshold is within this of its target


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "nb_tree_golden.npz"))


# ---- the exact value -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_exact_value_against_the_restatement_and_sklearn_on_the_golden_models(golden, name):
    """|exact - numpy in order| and |exact - scikit-learn| <= gnb_bound: the bound is between two fp64
    evaluations, the exact value lies at most half of it from each."""
    m = {k: golden["%s/%s" % (name, k)] for k in ("theta", "var", "class_prior", "classes")}
    m["name"] = "golden-" + name
    X = np.concatenate([golden[name + "/X"][::25], golden[name + "/tie_X"]])
    want = np.concatenate([golden[name + "/nb_jll"][::25], golden[name + "/tie_jll"]])
    exact, bound = E.exact_jll(m, X)[1], R.gnb_bound(m, X)
    for other in (R.gnb_jll(m, X), want):
        err = np.abs(exact - other)
        assert np.all(err <= bound) and np.all(err <= 0.5 * bound), (err / bound).max()
    # the near ties have margin 0 in scikit-learn's own scores, each within half a bound of exact: the exact
    # margin is at most (b_w + b_c) / 2, an eighth of the threshold
    for d, b in zip(E.exact_jll(m, golden[name + "/tie_X"])[0], R.gnb_bound(m, golden[name + "/tie_X"])):
        assert E.margin_ratio(d, b)[1] <= 0.5 / R.SAFETY


@pytest.mark.parametrize("C,D", [(3, 1), (3, 33), (64, 33), (3, 2049), (64, 4096)])
def test_exact_value_on_the_shape_models(C, D):
    m = E.shape_model(C, D)
    X = E.queries(m, 12, 7)
    rows = E.exact_rows(m, 12)
    assert len(rows) >= E.EXACT_MIN_ROWS and (len(rows) == 12 or C * D * len(rows) <= max(E.EXACT_BUDGET, 3 * C * D))
    X = X[rows]
    exact, bound = E.exact_jll(m, X)[1], R.gnb_bound(m, X)
    for other in (R.gnb_jll(m, X), E.as_sklearn(m)._joint_log_likelihood(X)):
        assert np.all(np.abs(exact - other) <= 0.5 * bound)
    assert np.array_equal(m["classes"][np.argmax(exact, axis=1)], E.as_sklearn(m).predict(X))


# ---- shapes ----------------------------------------------------------------------------------------
def test_shape_cases_hit_their_edges():
    form = E.kernel_form
    assert [form(3, D)[0] for D in (1, 2, 15, 16, 17, 31, 32, 33, 4096)] == [16, 16, 16, 16, 32, 32, 32, 0, 0]
    for D in E.DIMS:
        assert (E.DIM_C, D) in E.shape_cases()
    for D in (16, 17, 32, 33, 1024, 1025, 2047, 2048, 2049, 4095, 4096):
        assert D in E.DIMS
    # G whole classes per stage: 2 | 1 at D = 1024 | 1025; a class in 1 | 2 chunks at 2048 | 2049, 2 whole at 4096
    assert form(3, 1024)[2:] == (2, 2, 1) and form(3, 1025)[2:] == (1, 3, 1)
    assert form(3, 2047)[2:] == (1, 3, 1) and form(3, 2048)[2:] == (1, 3, 1) and form(3, 2049)[2:] == (1, 3, 2)
    assert form(3, 4095)[4] == 2 and form(3, 4096)[1:] == (2048, 1, 3, 2)
    # D = 33: 62 classes per stage -- one under, exactly one stage, one past, 64; D = 1024: one stage, one past
    assert [form(C, 33)[2:4] for C in (61, 62, 63, 64)] == [(62, 1), (62, 1), (62, 2), (62, 2)]
    assert [form(C, 1024)[2:4] for C in (2, 3)] == [(2, 1), (2, 2)]
    assert set(E.STAGE_CASES) == {(61, 33), (62, 33), (63, 33), (64, 33), (2, 1024), (3, 1024)}
    assert form(*E.CORNER) == (0, 2048, 1, 64, 2)
    # the register forms stage DP-wide rows: 128 | 64 classes a stage, so C <= 64 is one stage
    assert form(64, 16)[2:4] == (128, 1) and form(64, 32)[2:4] == (64, 1)
    T = E.GNB_T
    assert {0, 1, T - 1, T, T + 1, 2 * T + 1} == set(E.QUERY_COUNTS)
    for C, D in E.shape_cases():
        m = E.shape_model(C, D)
        assert m["theta"].shape == (C, D) and m["var"].min() > 0 and abs(m["class_prior"].sum() - 1) < 1e-12


def test_shape_queries_are_mostly_certifiable():
    """The shape tests certify every row at or above MUST thresholds; most rows must stand there."""
    for C, D in ((3, 2), (64, 33), (3, 1025)):
        m = E.shape_model(C, D)
        X = E.queries(m, 40, D)
        ratio = R.gnb_margin_ratio(R.gnb_jll(m, X), R.gnb_bound(m, X))
        assert (ratio >= 16.0).sum() >= 36, (C, D, np.sort(ratio)[:6])


# ---- the certificate -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,C,D,pair", E.band_cases(), ids=[c[0] for c in E.band_cases()])
def test_banded_queries_stand_where_they_claim(name, C, D, pair):
    _, m = E.fitted(C, D)
    assert m["theta"].shape == (C, D)
    X, ratio = E.banded_queries(m, pair)
    print(name, np.round(ratio, 4).tolist())
    targets = np.array(E.BAND_UNDER + E.BAND_OVER + (0.0, 0.0))
    assert X.shape == (len(targets), D)
    assert np.all(np.abs(ratio - targets) <= BAND_TOL * np.maximum(1.0, np.abs(targets))), ratio
    inside, outside = np.abs(ratio) <= E.MUST_NOT, np.abs(ratio) >= E.MUST
    assert inside.sum() == 6 and outside.sum() == 4 and np.all(inside[:4]) and np.all(outside[4:8])
    assert np.all(inside[8:]) and ratio[8] * ratio[9] <= 0  # the two doubles either side of the tie
    # both classes of the pair lead somewhere, and the rows differ in one coordinate alone
    assert (ratio > 0).any() and (ratio < 0).any()
    assert (np.ptp(X, axis=0) > 0).sum() == 1
    # the whole row: the exact winner is one of the pair, its margin the pair's
    for d, b, r in zip(E.exact_jll(m, X)[0], R.gnb_bound(m, X), ratio):
        w, worst = E.margin_ratio(d, b)
        assert w in pair and abs(worst - abs(r)) <= 1e-9 * max(1.0, abs(r))


def test_window_arithmetic():
    """A device score within one bound of exact on each side moves the margin by at most b_w + b_c, a quarter
    of the threshold: at most MUST_NOT + 1/4 < 1 thresholds, at least MUST - 1/4 > 1."""
    assert E.MUST_NOT + 1.0 / R.SAFETY < 1.0 < E.MUST - 1.0 / R.SAFETY
    assert max(abs(k) for k in E.BAND_UNDER) + BAND_TOL <= E.MUST_NOT
    assert min(abs(k) * (1 - BAND_TOL) if abs(k) > 2.5 else abs(k) - BAND_TOL for k in E.BAND_OVER) >= E.MUST


# ---- numeric ends ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.numeric_cases()))
def test_numeric_cases_hit_their_edges(name):
    """The outcome written beside each case is the restatement's, and the exact value's where one exists."""
    m, X, cert, pred = E.numeric_cases()[name]
    with np.errstate(all="ignore"):
        jll, bound = R.gnb_jll(m, X), R.gnb_bound(m, X)
        got = R.gnb_certified(jll, bound)
    assert np.array_equal(got.astype(np.int32), cert), (got, cert)
    stated = pred >= 0
    assert np.array_equal(np.argmax(jll, axis=1)[stated], pred[stated])
    if np.isfinite(m["theta"]).all() and np.isfinite(m["var"]).all():
        exact = E.exact_jll(m, X)
        for i, (d, b) in enumerate(zip(exact[0], bound)):
            if not np.isfinite(exact[1][i]).all() or not np.isfinite(jll[i]).all():
                assert cert[i] == 0  # a score that is not finite (in fp64: an overflowing square or quotient)
                continue
            w, ratio = E.margin_ratio(d, b)
            if cert[i]:
                assert ratio >= E.MUST and w == np.argmax(jll[i]), (i, ratio)
            else:
                assert ratio <= E.MUST_NOT, (i, ratio)  # a finite uncertified row is a tie
    shape = {"var_1e-300": lambda: m["var"][1].max() == 1e-300 and np.isneginf(jll[3, 1]) and jll[2, 1] > 1700,
             "var_1e300": lambda: m["var"][1].min() == 1e300 and np.all(jll[:, 1] < -1700),
             "var_subnormal": lambda: 0 < m["var"][1].max() < np.finfo(np.float64).tiny and np.isneginf(jll[0, 1]),
             "theta_1e+150": lambda: np.isfinite(jll).all() and jll[:, 1].max() < -1e299,
             "theta_-1e+150": lambda: np.isfinite(jll).all() and jll[:, 1].max() < -1e299,
             "theta_1e+300": lambda: np.all(np.isneginf(jll[:, 1])) and np.isfinite(jll[:, [0, 2]]).all(),
             "theta_-1e+300": lambda: np.all(np.isneginf(jll[:, 1])) and np.isfinite(jll[:, [0, 2]]).all(),
             "partial_inf": lambda: np.all(np.isneginf(jll[:, 0])) and np.isfinite(jll[:, 1:]).all(),
             "duplicate_classes": lambda: np.array_equal(jll[:, 0].view(np.uint64), jll[:, 2].view(np.uint64)),
             "two_equal_classes": lambda: np.array_equal(jll[:, 0].view(np.uint64), jll[:, 1].view(np.uint64)),
             "exact_tie": lambda: np.array_equal(jll[:2, 0].view(np.uint64), jll[:2, 1].view(np.uint64)),
             "nan_class_0": lambda: np.isnan(jll[:, 0]).all() and np.isfinite(jll[:, 1:]).all(),
             "nan_class_1": lambda: np.isnan(jll[:, 1]).all() and np.isfinite(jll[:, [0, 2]]).all(),
             "zero_prior_0": lambda: np.all(np.isneginf(jll[:, 0])) and np.isfinite(jll[:, 1:]).all(),
             "zero_prior_2": lambda: np.all(np.isneginf(jll[:, 2])) and np.isfinite(jll[:, :2]).all(),
             "one_class": lambda: jll.shape == (3, 1) and np.isneginf(jll[2, 0])}
    assert shape[name](), name


def test_scikit_learn_refuses_rows_that_are_not_finite_and_takes_huge_ones():
    nb, m = E.fitted(3, 40)
    X = E.queries(m, 5, 3)
    for bad in E.NONFINITE:
        Q = X.copy()
        Q[2, 39] = bad
        with pytest.raises(ValueError):
            nb.predict(Q)
    Q = X.copy()
    Q[2, 39] = E.HUGE
    with np.errstate(all="ignore"):
        assert nb.predict(Q).shape == (5,) and np.all(np.isneginf(R.gnb_jll(m, Q)[2]))
    cells = E.nonfinite_cells(40)
    assert {c for _, c in cells} == {0, 33, 39} and {128, 127} <= {r for r, _ in cells}
    assert {c for _, c in E.nonfinite_cells(5)} == {0, 4}


# ---- trees -----------------------------------------------------------------------------------------
def test_tree_tables_hit_their_edges():
    from src import _hip
    lds = _hip.load_library().dsp_tree_lds_nodes()
    assert lds == E.TREE_LDS_NODES == 4096
    for n, extra, depth in ((4095, 0, 2047), (4095, 1, 2047), (4097, 0, 2048)):
        t = E.chain_tree(n, extra)
        assert len(t["left"]) == n + extra and t["max_depth"] == depth
        assert (len(t["left"]) <= lds) == (n == 4095) and (n + extra == lds) == (extra == 1)
        assert 16 * len(t["left"]) <= 65536 or n == 4097  # exactly 64 KiB of nodes at 4096
        X = E.chain_queries(depth, 257)
        assert X[:5, 0].tolist() == [0, depth - 2, depth - 1, depth, depth + 1]
        for md in (depth, depth - 1):
            want = E.chain_leaf(depth, X, md)
            pred, leaf = R.tree_walk(dict(t, max_depth=md), X)
            assert np.array_equal(leaf, want)
            assert np.array_equal(pred, np.where(want >= 0, want % 7, -1))
            assert (want[:5] < 0).tolist() == [False, False] + [md < depth] * 3
        assert not np.isin(np.arange(n, n + extra), E.chain_leaf(depth, X, depth)).any()  # unreachable
    T = E.TREE_T
    assert set(E.TREE_QUERY_COUNTS) == {0, 1, T - 1, T, T + 1}


def test_stumps_hit_their_edges():
    f32 = E.F32
    t = E.THRESHOLDS
    assert f32(E.SUB_MIN) > 0 and f32(E.SUB_MIN) / f32(2) == 0 and f32(0.5 * E.SUB_MIN) == 0  # (ties to even)
    for v in (1e-40, 1.5e-40):
        assert 0 < float(f32(v)) < float(np.finfo(f32).tiny) and float(f32(v)) != v
    assert f32(1e-50) == 0 and f32(-1e-50) == 0 and f32(1e-46) == 0 and np.signbit(f32(-1e-46))
    with np.errstate(over="ignore"):
        assert f32(t[9]) == f32(E.FLT_MAX) and t[9] > E.FLT_MAX and f32(t[10]) == f32(E.FLT_MAX) and t[10] < E.FLT_MAX
        assert np.isposinf(f32(E.MIDPOINT)) and np.isposinf(f32(np.nextafter(E.MIDPOINT, np.inf)))
        assert f32(np.nextafter(E.MIDPOINT, 0.0)) == f32(E.FLT_MAX)
        assert np.isposinf(f32(1e40)) and np.isneginf(f32(-1e40))
    assert E.MIDPOINT == (E.FLT_MAX + 2.0 ** 128) / 2
    assert len(set(map(repr, t))) == len(t) == 16 and sum(np.isnan(x) for x in t) == 1
    for thr in t:
        vals = E.stump_values(thr)
        want = E.stump_leaf(thr, vals)
        pred, leaf = R.tree_walk(E.stump(thr), vals[:, None])
        assert np.array_equal(leaf, want), thr
        assert np.array_equal(pred, np.where(want < 0, -1, want - 1))
        assert (want < 0).sum() >= 3  # the midpoint, its upper neighbour and -midpoint at least
        if abs(thr) < 1e38:
            assert {1, 2} <= set(want.tolist()), thr  # the values stand on both sides
    # the decisions float_below exists for, stated outright
    def leaf(thr, x):
        return int(E.stump_leaf(thr, [x])[0])
    assert leaf(-1e-50, 0.0) == 2 and leaf(-1e-50, -0.0) == 2 and leaf(-1e-50, -E.SUB_MIN) == 1
    assert leaf(1e-50, 0.0) == 1 and leaf(1e-50, E.SUB_MIN) == 2
    assert leaf(0.5 * E.SUB_MIN, E.SUB_MIN) == 2 and leaf(0.5 * E.SUB_MIN, 1e-46) == 1
    assert leaf(0.0, -0.0) == 1 and leaf(-0.0, 0.0) == 1 and leaf(0.0, E.SUB_MIN) == 2
    assert leaf(1e40, E.FLT_MAX) == 1 and leaf(-1e40, -E.FLT_MAX) == 2 and leaf(t[10], E.FLT_MAX) == 2
    assert leaf(np.inf, E.FLT_MAX) == 1 and leaf(-np.inf, -E.FLT_MAX) == 2 and leaf(np.nan, 0.0) == 2
    assert leaf(1e40, E.MIDPOINT) == -1 and leaf(1e40, float(np.nextafter(E.MIDPOINT, 0.0))) == 1


@pytest.mark.parametrize("seed", [1, 2])
def test_walk_restatement_is_sklearns_on_subnormal_thresholds(seed):
    tree, Q = E.subnormal_tree(seed)
    tiny = float(np.finfo(E.F32).tiny)
    inner = tree.tree_.children_left != -1
    thr = tree.tree_.threshold[inner]
    assert inner.sum() >= 5 and np.all(np.abs(thr) < tiny) and np.all(thr != 0) and (thr < 0).any() and (thr > 0).any()
    assert np.all(np.abs(Q) < tiny)
    t = R.tree_arrays(tree)
    pred, leaf = R.tree_walk(t, Q)
    assert np.array_equal(leaf, tree.apply(Q)) and np.array_equal(t["classes"][pred], tree.predict(Q))
    # a flushed subnormal would change decisions: with every value and threshold flushed to zero the leaves differ
    flushed = dict(t, threshold=np.zeros_like(t["threshold"]))
    assert not np.array_equal(R.tree_walk(flushed, np.zeros_like(Q))[1], leaf)


# ---- fit -------------------------------------------------------------------------------------------
def test_fit_cases_hit_their_edges():
    cases = E.fit_shape_cases()
    assert {n for n, _, _ in cases} >= set(E.FIT_N) and {d for _, d, _ in cases} >= set(E.FIT_D)
    assert {c for _, _, c in cases} >= set(E.FIT_C) and E.FIT_WIDE in cases and E.FIT_WIDE[:2] == (9, 4096)
    assert {7, 8, 9, 127, 128, 129, 255, 256, 257} <= set(E.FIT_N)  # the batch of 8 and the tile of 128
    assert {15, 16, 17, 32, 33} <= set(E.FIT_D) and {7, 8, 15, 16, 63, 64} <= set(E.FIT_C)
    for N, D, C in cases:
        X, y = E.fit_data(N, D, C)
        assert X.shape == (N, D) and y.shape == (N,) and len(np.unique(y)) == min(N, C) and y.max() < C
    v = E.fit_value_cases()
    for name, gone in (("empty_first", 0), ("empty_middle", 4), ("empty_last", 8)):
        assert gone not in v[name][1] and len(np.unique(v[name][1])) == 8 and not v[name][3]
    Z = v["minus_zero_column"][0]
    assert np.all(np.signbit(Z[:, [3, 16]])) and np.all(Z[:, [3, 16]] == 0)
    assert not v["nan_and_inf"][3] and np.isnan(v["nan_and_inf"][0][:, 7]).sum() == 1


@pytest.mark.parametrize("N,D,C", E.fit_shape_cases())
def test_fit_restatement_is_sklearns_on_the_shape_cases(N, D, C):
    from sklearn.naive_bayes import GaussianNB
    X, y = E.fit_data(N, D, C)
    nb = GaussianNB().fit(X, y)
    theta, var, count, eps = R.gnb_fit(X, y, C)
    if N >= C:
        assert E.same_values(theta, nb.theta_) and E.same_values(var, nb.var_) and E.same_values(eps, nb.epsilon_)
        assert np.array_equal(count.astype(np.float64), nb.class_count_)
    else:  # scikit-learn sees only the classes present
        assert E.same_values(theta[:N], nb.theta_) and E.same_values(var[:N], nb.var_)


@pytest.mark.parametrize("name", list(E.fit_value_cases()))
def test_fit_restatement_on_the_value_cases(name):
    from sklearn.naive_bayes import GaussianNB
    X, y, C, accepted = E.fit_value_cases()[name]
    with np.errstate(all="ignore"):
        theta, var, count, eps = R.gnb_fit(X, y, C)
    if accepted:
        with np.errstate(all="ignore"):
            nb = GaussianNB().fit(X, y)
        assert E.same_values(theta, nb.theta_) and E.same_values(var, nb.var_) and E.same_values(eps, nb.epsilon_)
        assert np.array_equal(count.astype(np.float64), nb.class_count_)
    if name.startswith("empty"):
        gone = int(np.flatnonzero(count == 0)[0])
        keep = np.arange(C) != gone
        assert np.isnan(theta[gone]).all() and np.isnan(var[gone]).all() and keep.sum() == 8
        nb = GaussianNB().fit(X, y)  # the classes present are scikit-learn's
        assert E.same_values(theta[keep], nb.theta_) and E.same_values(var[keep], nb.var_) and eps == nb.epsilon_
    if name == "minus_zero_column":
        # np.add.reduce adds the rows to +0.0: the mean of -0.0 alone is +0.0
        assert not np.signbit(theta[:, [3, 16]]).any() and np.all(theta[:, [3, 16]] == 0) and np.all(var[:, [3, 16]] == eps)
    if name == "constant_within_class":
        assert np.all(var[:, 5] == eps) and np.array_equal(theta[:, 5], np.arange(9) * 0.5 + 1.0)
    if name == "squares_overflow":
        assert np.isposinf(eps) and np.all(np.isposinf(var)) and np.isfinite(theta).all()
    if name == "nan_and_inf":
        with pytest.raises(ValueError):
            GaussianNB().fit(X, y)
        assert np.isnan(eps) and np.isnan(var).all() and np.isfinite(theta[:, :7]).all()
