"""dsp_gnb_predict, dsp_gnb_fit (csrc/gnb.hip) and dsp_tree_predict (csrc/tree.hip) at their shape and
numeric edges (tests/nb_tree_edge_cases.py), through the bare C ABI: 64 NaNs stand behind every
floating-point input and 1 << 20 behind every integer one, so a read past an array shows in the results;
every output lies between guard rows (tests/device_outputs.py), and the workspace starts as garbage, so a
counter nobody cleared shows too.

The tolerance on jll is the project's derived bound (tests/nb_tree_reference.gnb_bound)
against the exact decimal value (nb_tree_edge_cases.exact_jll) on the rows exact_rows picks, and against
scikit-learn's _joint_log_likelihood and the numpy restatement -- two more fp64 evaluations, which the
bound is about -- on all of them.  Every check prints its largest err / bound.  Everything else is exact."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nb_tree_edge_cases as E
import nb_tree_reference as R
from device_outputs import Guarded, bits

pytestmark = pytest.mark.gpu

FILL = -5
TAIL = 64
JUNK = 0x5A  # what the workspace, its counter included, holds before a call


def _behind(a, np_dtype, tail):
    a = np.asarray(a, np_dtype).ravel()
    return torch.as_tensor(np.concatenate([a, np.full(TAIL, tail, np_dtype)])).to("cuda")


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


class _Launch:
    """What the three calls' buffers share: the library, a workspace of garbage, guarded outputs."""

    def __init__(self, nbytes, short=0):
        from src import _hip
        self.lib, self.hip = _hip.lib(), _hip
        assert nbytes > 0
        self.nbytes = nbytes - short
        self.ws = torch.full((nbytes,), JUNK, dtype=torch.uint8, device="cuda")
        self.outs = []

    def out(self, shape, dtype, fill=FILL):
        g = Guarded(shape, dtype, FILL if dtype.is_floating_point is False else float(FILL))
        g.inside = fill
        if fill != FILL:
            g.view.fill_(fill)
        self.outs.append(g)
        return g

    def refill(self):
        for g in self.outs:
            g.view.fill_(g.inside)
        self.ws[:4] = JUNK

    def counter(self):
        return int(self.ws[:4].view(torch.int32).item())

    def untouched(self):
        torch.cuda.synchronize()
        return all(np.array_equal(g.get(), np.full(g.view.shape, g.inside), equal_nan=True) for g in self.outs)


class NbLaunch(_Launch):
    """One dsp_gnb_predict call's buffers.  The keyword arguments replace what the model says."""

    def __init__(self, m, X, with_jll=True, D=None, C=None, Nq=None, null=None, short=0):
        from src import _hip
        X = np.ascontiguousarray(X, np.float64)
        c, d = m["theta"].shape
        self.rows = X.shape[0]
        super().__init__(_hip.lib().dsp_gnb_workspace_bytes(self.rows, d, c), short)
        self.D, self.C, self.Nq = d if D is None else D, c if C is None else C, self.rows if Nq is None else Nq
        lp, nc = E.constants(m)
        self.model = [None if null == k else _behind(a, np.float64, np.nan)
                      for k, a in (("theta", m["theta"]), ("var", m["var"]), ("log_prior", lp), ("nconst", nc))]
        self.q = _behind(X, np.float64, np.nan)
        self.pred = self.out((self.rows,), torch.int32)
        self.jll = self.out((self.rows, c), torch.float64) if with_jll else None
        self.cert = self.out((self.rows,), torch.int32)

    def call(self):
        p = self.hip.ptr
        return self.lib.dsp_gnb_predict(*[None if t is None else p(t) for t in self.model], self.D, self.C, p(self.q),
                                        self.Nq, p(self.pred.view), p(self.jll.view) if self.jll else None,
                                        p(self.cert.view), p(self.ws), self.nbytes, self.hip.stream_handle())

    def read(self):
        """(the guards are checked by Guarded.get)"""
        torch.cuda.synchronize()
        return SimpleNamespace(pred=self.pred.get(), cert=self.cert.get(), jll=self.jll.get() if self.jll else None,
                               unc=self.counter())


def run_nb(m, X, **kw):
    L = NbLaunch(m, X, **kw)
    rc = L.call()
    assert rc == 0, rc
    return L.read()


def nb_reference(m, X):
    """What a model's rows are compared with, computed once and sliced by the checks that launch a part of
    X: scikit-learn's and the restatement's jll, the bound, and on exact_rows the exact decimals."""
    with np.errstate(all="ignore"):
        ref = SimpleNamespace(sk=E.as_sklearn(m)._joint_log_likelihood(X), np_=R.gnb_jll(m, X), bound=R.gnb_bound(m, X))
    ref.rows = E.exact_rows(m, len(X))
    ref.dec, ref.exact = E.exact_jll(m, X[ref.rows])
    ref.label = m["classes"][np.argmax(ref.sk, axis=1)]  # GaussianNB.predict: classes_[argmax of its jll]
    return ref


WORST = {"err/bound": 0.0}


def check_nb(tag, m, r, ref, n=None):
    """jll within the bound of the exact value, of scikit-learn's and of the restatement's; the label is
    the exact argmax wherever the exact margin exceeds the two bounds; every row MUST thresholds out is
    certified, none inside MUST_NOT is; a certified label is the exact argmax and scikit-learn's; the
    counter is the number of uncertified rows."""
    n = len(r.pred) if n is None else n
    assert len(r.pred) == n and r.jll.shape == (n, len(m["classes"]))
    assert set(np.unique(r.cert)) <= {0, 1} and r.unc == int((r.cert == 0).sum())
    if n == 0:
        return 0.0
    assert not np.isnan(r.jll).any(), "a read past an input array"
    bound = ref.bound[:n]
    rows = ref.rows[ref.rows < n]
    worst = 0.0
    for name, want, at in (("exact", ref.exact[:len(rows)], rows), ("sklearn", ref.sk[:n], slice(None)),
                           ("numpy", ref.np_[:n], slice(None))):
        err = np.abs(r.jll[at] - want) / bound[at]
        assert np.all(err <= 1.0), (tag, name, err.max())
        worst = max(worst, float(err.max()))
    assert r.pred.min() >= 0 and r.pred.max() < len(m["classes"])
    # the exact rows: winner and margin in thresholds from the decimals
    for i, d in zip(rows, ref.dec):
        w, ratio = E.margin_ratio(d, bound[i])
        if ratio > 1.0 / R.SAFETY:  # beyond the two bounds: the device's largest score is the exact one's
            assert r.pred[i] == w, (tag, i, ratio)
        assert not (ratio >= E.MUST and r.cert[i] == 0) and not (ratio <= E.MUST_NOT and r.cert[i] == 1), (tag, i, ratio)
        assert r.cert[i] == 0 or r.pred[i] == w
    # every row: the same against the restatement, which the device is within one bound of
    ratio = R.gnb_margin_ratio(ref.np_[:n], bound)
    clear = ratio > 2.0 / R.SAFETY
    assert np.array_equal(r.pred[clear], np.argmax(ref.np_[:n], axis=1)[clear])
    assert np.all(r.cert[ratio >= E.MUST + 0.5] == 1) and np.all(r.cert[ratio <= E.MUST_NOT - 0.25] == 0)
    won = r.cert == 1
    assert np.all(ratio[won] > 0.5) and np.array_equal(m["classes"][r.pred[won]], ref.label[:n][won])
    WORST["err/bound"] = max(WORST["err/bound"], worst)
    print("%s: max err / bound %.3g (largest so far %.3g), certified %d of %d, min margin / threshold %.3g"
          % (tag, worst, WORST["err/bound"], int(won.sum()), n, ratio.min()))
    return worst


# ---- dsp_gnb_predict: shapes -------------------------------------------------------------------------
@pytest.mark.parametrize("C,D", E.shape_cases())
def test_nb_dimension_class_and_row_count_edges(C, D):
    """Either side of every kernel form, stage size and chunk count, at Nq = 0, 1, 127, 128, 129, 257: row 0
    keeps its bits alone, in every batch, as the last lane of a full workgroup and as the row the idle lanes
    of a workgroup shadow; jll = NULL changes neither labels nor certificates."""
    m = E.shape_model(C, D)
    X = E.queries(m, max(E.QUERY_COUNTS), 31 * C + D)
    ref = nb_reference(m, X)
    row0 = None
    for n in E.QUERY_COUNTS:
        r = run_nb(m, X[:n])
        check_nb("C=%d D=%d Nq=%d" % (C, D, n), m, r, ref, n)
        if n == 0:
            assert r.unc == 0  # (the workspace held garbage)
            continue
        row0 = r if row0 is None else row0
        assert same_bits(r.jll[0], row0.jll[0]) and r.pred[0] == row0.pred[0] and r.cert[0] == row0.cert[0], n
        if n in (E.GNB_T, E.GNB_T + 1):
            moved = run_nb(m, np.concatenate([X[1:n], X[:1]]))
            assert same_bits(moved.jll[-1], row0.jll[0]) and moved.pred[-1] == row0.pred[0], n
            assert same_bits(moved.jll[:-1], r.jll[1:]) and np.array_equal(moved.cert[:-1], r.cert[1:])
    bare = run_nb(m, X, with_jll=False)
    assert bare.jll is None and np.array_equal(bare.pred, r.pred) and np.array_equal(bare.cert, r.cert) and bare.unc == r.unc
    assert int((r.cert == 1).sum()) >= len(X) - 8  # (the rows are ordinary: nearly all are certified)


# ---- dsp_gnb_predict: the certificate -----------------------------------------------------------------
@pytest.mark.parametrize("name,C,D,pair", E.band_cases(), ids=[c[0] for c in E.band_cases()])
def test_nb_certificate_threshold(name, C, D, pair):
    """Rows whose exact margin between the two leading classes stands at chosen multiples of the threshold
    SAFETY (bound_w + bound_c), every other class decided.  The device's scores are within one bound of
    exact on each side, so a row at most 0.5 thresholds out must not be certified (the two doubles either
    side of the tie among them) and a row 2 or more out must be; no row is left out, the counter is the
    number of uncertified rows, and a certified label is the exact argmax and scikit-learn's."""
    nb, m = E.fitted(C, D)
    X, ratio = E.banded_queries(m, pair)
    dec, exact = E.exact_jll(m, X)
    bound = R.gnb_bound(m, X)
    r = run_nb(m, X)
    err = np.abs(r.jll - exact) / bound
    sk_err = np.abs(r.jll - nb._joint_log_likelihood(X)) / bound
    print("%s: exact margin / threshold %s, certified %s, max err / bound %.3g (scikit-learn %.3g)"
          % (name, np.round(ratio, 3).tolist(), r.cert.tolist(), err.max(), sk_err.max()))
    WORST["err/bound"] = max(WORST["err/bound"], float(err.max()), float(sk_err.max()))
    assert np.all(err <= 1.0) and np.all(sk_err <= 1.0)
    inside, outside = np.abs(ratio) <= E.MUST_NOT, np.abs(ratio) >= E.MUST
    assert inside.sum() == 6 and outside.sum() == 4 and np.all(inside | outside)  # every row stands under a rule
    assert np.all(r.cert[inside] == 0), (ratio, r.cert)
    assert np.all(r.cert[outside] == 1), (ratio, r.cert)
    assert r.unc == 6
    won = r.cert == 1
    want = np.array([E.margin_ratio(d, b)[0] for d, b in zip(dec, bound)])
    assert np.array_equal(r.pred[won], want[won]) and np.array_equal(want[won], np.where(ratio > 0, *pair)[won])
    assert np.array_equal(m["classes"][r.pred[won]], nb.predict(X)[won])
    assert np.all(np.isin(r.pred, pair))


# ---- dsp_gnb_predict: numeric ends -----------------------------------------------------------------------
def _classifier(kind, model):
    from src.models import TraditionalClassifier
    clf = TraditionalClassifier(kind)
    clf.model = model
    return clf


def _outcome(fn, X):
    """('ok', result) or ('raises', the exception's type)."""
    try:
        with np.errstate(all="ignore"):
            return "ok", fn(X)
    except Exception as e:  # noqa: BLE001 -- whatever the model raises is what the classifier must raise
        return "raises", type(e)


def same_outcome(ours, theirs, X):
    a, b = _outcome(ours, X), _outcome(theirs, X)
    return a[0] == b[0] and (np.array_equal(a[1], b[1]) if a[0] == "ok" else a[1] is b[1])


@pytest.mark.parametrize("name", list(E.numeric_cases()))
def test_nb_numeric_ends(name):
    """The certificate and, where it is stated, the label are the ones written beside the case
    (nb_tree_edge_cases.numeric_cases, pinned against the restatement and the exact value by the host test);
    a score is finite, -inf or NaN exactly where the restatement's is, and within the bound where finite; the
    classifier's labels are scikit-learn's."""
    m, X, cert, pred = E.numeric_cases()[name]
    r = run_nb(m, X)
    with np.errstate(all="ignore"):
        jll, bound = R.gnb_jll(m, X), R.gnb_bound(m, X)
    print(name, "certified", r.cert.tolist(), "pred", r.pred.tolist())
    assert np.array_equal(r.cert, cert) and r.unc == int((cert == 0).sum())
    stated = pred >= 0
    assert np.array_equal(r.pred[stated], pred[stated])
    assert np.array_equal(np.isnan(r.jll), np.isnan(jll)) and np.array_equal(np.isneginf(r.jll), np.isneginf(jll))
    assert not np.isposinf(r.jll).any()
    fin = np.isfinite(jll)
    assert np.all(np.abs(r.jll[fin] - jll[fin]) <= bound[fin])
    won = r.cert == 1
    assert np.array_equal(r.pred[won], np.argmax(jll, axis=1)[won])
    sk = E.as_sklearn(m)
    clf = _classifier('naive_bayes', sk)
    assert same_outcome(clf.predict, sk.predict, X)
    assert clf.last_predict_stats == {'device': True, 'uncertified': int((cert == 0).sum())}


def nonfinite_models():
    return [("d5", E.hand_model(3, 5, 11, name="numeric")), ("d40", E.fitted(3, 40)[1])]


@pytest.mark.parametrize("bad", E.NONFINITE + (E.HUGE,), ids=str)
@pytest.mark.parametrize("case", nonfinite_models(), ids=lambda c: c[0])
def test_nb_rows_that_are_not_finite_are_uncertified(case, bad):
    """NaN, +-inf and 1.7e308 (finite, its square is not) in the first column, the last and one past 32, in
    the last lane of a full workgroup and in the row idle lanes shadow: never certified, counted, NaN or
    -inf in every score; every other row keeps its bits.  The classifier raises where scikit-learn does."""
    _, m = case
    D = m["theta"].shape[1]
    X = E.queries(m, 129, 14)
    clean = run_nb(m, X)
    Xb = X.copy()
    cells = E.nonfinite_cells(D)
    for r_, c_ in cells:
        Xb[r_, c_] = bad
    rows = np.array(sorted({r_ for r_, _ in cells}))
    r = run_nb(m, Xb)
    expected = int(((clean.cert == 0) | np.isin(np.arange(129), rows)).sum())
    assert np.all(r.cert[rows] == 0) and r.unc == expected
    assert np.all(np.isnan(r.jll[rows]) if np.isnan(bad) else np.isneginf(r.jll[rows]))
    keep = np.setdiff1d(np.arange(129), rows)
    assert same_bits(r.jll[keep], clean.jll[keep]) and np.array_equal(r.pred[keep], clean.pred[keep])
    assert np.array_equal(r.cert[keep], clean.cert[keep]) and clean.unc <= 2
    sk = E.as_sklearn(m)
    clf = _classifier('naive_bayes', sk)
    if np.isfinite(bad):
        assert np.array_equal(clf.predict(Xb), sk.predict(Xb))  # scikit-learn takes the huge rows: its labels
    else:
        with pytest.raises(ValueError):
            sk.predict(Xb)
        with pytest.raises(ValueError):
            clf.predict(Xb)
    assert clf.last_predict_stats == {'device': True, 'uncertified': expected}


# ---- dsp_gnb_predict: arguments -----------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(D=0), dict(D=4097), dict(C=0), dict(C=65), dict(Nq=-1), dict(null="theta"),
                                dict(null="var"), dict(null="log_prior"), dict(null="nconst"), dict(short=1)], ids=str)
def test_nb_rejected_arguments_touch_nothing(kw):
    from src import _hip
    m = E.shape_model(3, 17)
    L = NbLaunch(m, E.queries(m, 7, 4), **kw)
    assert L.call() == (_hip.DSP_ERR_WORKSPACE if "short" in kw else _hip.DSP_ERR_ARGS)
    assert L.untouched() and L.counter() == int.from_bytes(bytes([JUNK] * 4), "little")


# ---- dsp_gnb_fit ---------------------------------------------------------------------------------------
class FitLaunch(_Launch):
    """One dsp_gnb_fit call's buffers: NaN in theta, var and epsilon and -1 in class_count between the guard
    rows, so an element nobody wrote shows."""

    def __init__(self, X, y, C, var_smoothing=1e-9):
        X = np.ascontiguousarray(X, np.float64)
        self.N, self.D = X.shape
        super().__init__(8 * self.D)
        self.C, self.vs = C, var_smoothing
        self.X, self.y = _behind(X, np.float64, np.nan), _behind(y, np.int32, 1 << 20)
        self.theta = self.out((C, self.D), torch.float64, float("nan"))
        self.var = self.out((C, self.D), torch.float64, float("nan"))
        self.count = self.out((C,), torch.int64, -1)
        self.eps = self.out((1,), torch.float64, float("nan"))

    def call(self):
        p = self.hip.ptr
        return self.lib.dsp_gnb_fit(p(self.X), p(self.y), self.N, self.D, self.C, self.vs, p(self.theta.view),
                                    p(self.var.view), p(self.count.view), p(self.eps.view), p(self.ws), self.nbytes,
                                    self.hip.stream_handle())

    def read(self):
        torch.cuda.synchronize()
        return self.theta.get(), self.var.get(), self.count.get(), float(self.eps.get()[0])


def run_fit(X, y, C):
    L = FitLaunch(X, y, C)
    rc = L.call()
    assert rc == 0, rc
    return L.read()


@pytest.mark.parametrize("N,D,C", E.fit_shape_cases())
def test_fit_shape_edges_equal_sklearn_bit_for_bit(N, D, C):
    """The tile of 128 rows, the batch of 8, the 16 columns and the 8 class slots of a workgroup, each from
    one under to one over; every element written."""
    from sklearn.naive_bayes import GaussianNB
    X, y = E.fit_data(N, D, C)
    nb = GaussianNB().fit(X, y)
    theta, var, count, eps = run_fit(X, y, C)
    assert E.same_values(theta, nb.theta_) and E.same_values(var, nb.var_) and E.same_values(eps, nb.epsilon_)
    assert not np.isnan(theta).any() and not np.isnan(var).any()
    assert np.array_equal(count.astype(np.float64), nb.class_count_)


@pytest.mark.parametrize("name", list(E.fit_value_cases()))
def test_fit_value_edges(name):
    """A class without rows in the first, a middle and the last slot (count 0, NaN rows: the header's stated
    result), columns of -0.0 (the mean is +0.0, as np.add.reduce's), a column constant within each class,
    squares that overflow, a NaN and an inf that poison epsilon: scikit-learn's bits where it has an answer,
    the restatement's where it has none."""
    from sklearn.naive_bayes import GaussianNB
    X, y, C, accepted = E.fit_value_cases()[name]
    theta, var, count, eps = run_fit(X, y, C)
    with np.errstate(all="ignore"):
        want = R.gnb_fit(X, y, C)
        if accepted:
            nb = GaussianNB().fit(X, y)
            want = (nb.theta_, nb.var_, nb.class_count_.astype(np.int64), nb.epsilon_)
    assert E.same_values(theta, want[0]) and E.same_values(var, want[1]) and E.same_values(eps, want[3])
    assert np.array_equal(count, want[2])
    if name.startswith("empty"):
        gone = {"empty_first": 0, "empty_middle": 4, "empty_last": 8}[name]
        assert count[gone] == 0 and np.isnan(theta[gone]).all() and np.isnan(var[gone]).all()
        assert np.isfinite(np.delete(theta, gone, axis=0)).all() and np.isfinite(np.delete(var, gone, axis=0)).all()
    if name == "minus_zero_column":
        assert same_bits(theta[:, [3, 16]], np.zeros((C, 2)))


# ---- dsp_tree_predict ------------------------------------------------------------------------------------
class TreeLaunch(_Launch):
    """One dsp_tree_predict call's buffers.  The keyword arguments replace what the table says."""

    def __init__(self, t, X, with_leaf=True, max_depth=None, D=None, n_nodes=None, Nq=None, null=None, short=0):
        from src import _hip
        X = np.ascontiguousarray(X, np.float64)
        n = len(t["left"])
        self.rows = X.shape[0]
        super().__init__(_hip.lib().dsp_tree_workspace_bytes(n), short)
        self.n = n if n_nodes is None else n_nodes
        self.D, self.Nq = X.shape[1] if D is None else D, self.rows if Nq is None else Nq
        self.depth = int(t["max_depth"]) if max_depth is None else max_depth
        self.table = [None if null == k else _behind(t[k], dt, tail) for k, dt, tail in
                      (("left", np.int32, 1 << 20), ("right", np.int32, 1 << 20), ("feature", np.int32, 1 << 20),
                       ("threshold", np.float64, np.nan), ("leaf_class", np.int32, 1 << 20))]
        self.q = _behind(X, np.float64, np.nan)
        self.pred = self.out((self.rows,), torch.int32)
        self.leaf = self.out((self.rows,), torch.int32) if with_leaf else None

    def call(self):
        p = self.hip.ptr
        return self.lib.dsp_tree_predict(*[None if a is None else p(a) for a in self.table], self.n, self.depth, self.D,
                                         p(self.q), self.Nq, p(self.pred.view), p(self.leaf.view) if self.leaf else None,
                                         p(self.ws), self.nbytes, self.hip.stream_handle())

    def read(self):
        torch.cuda.synchronize()
        return SimpleNamespace(pred=self.pred.get(), leaf=self.leaf.get() if self.leaf else None, bad=self.counter())


def run_tree(t, X, **kw):
    L = TreeLaunch(t, X, **kw)
    rc = L.call()
    assert rc == 0, rc
    return L.read()


def check_tree(t, X, want_leaf, **kw):
    """leaf and pred exact, the counter the number of rows answered -1, leaf = NULL the same labels."""
    r = run_tree(t, X, **kw)
    assert np.array_equal(r.leaf, want_leaf), np.flatnonzero(r.leaf != want_leaf)[:8]
    assert np.array_equal(r.pred, np.where(want_leaf >= 0, t["leaf_class"][np.maximum(want_leaf, 0)], -1))
    assert r.bad == int((want_leaf < 0).sum())
    bare = run_tree(t, X, with_leaf=False, **kw)
    assert bare.leaf is None and np.array_equal(bare.pred, r.pred) and bare.bad == r.bad
    return r


@pytest.fixture(scope="module")
def chains():
    """name -> (table, depth, rows, the restatement's leaves at max_depth = depth and depth - 1)."""
    out = {}
    for name, n, extra in (("4095", 4095, 0), ("4096", 4095, 1), ("4097", 4097, 0)):
        t = E.chain_tree(n, extra)
        depth = int(t["max_depth"])
        X = E.chain_queries(depth, 257)
        out[name] = (t, depth, X, [R.tree_walk(dict(t, max_depth=md), X)[1] for md in (depth, depth - 1)])
    return out


@pytest.mark.parametrize("name", ["4095", "4096", "4097"])
def test_tree_tables_around_the_lds_limit(chains, name):
    """Chains of 4095 and 4097 nodes (the LDS-resident and the memory walk) and the table of exactly 4096
    nodes, 64 KiB of dynamic LDS: the restatement's leaves and the contract's own, at max_depth equal to the
    depth and one below it (the deepest leaves are then cut)."""
    from src import _hip
    t, depth, X, walks = chains[name]
    lds = _hip.lib().dsp_tree_lds_nodes()
    assert (len(t["left"]) <= lds) == (name != "4097") and (len(t["left"]) == lds) == (name == "4096")
    for md, want in zip((depth, depth - 1), walks):
        assert np.array_equal(want, E.chain_leaf(depth, X, md))
        r = check_tree(t, X, want, max_depth=md)
        assert (r.leaf[:5] < 0).tolist() == [False, False] + [md < depth] * 3


def test_tree_lds_walk_and_memory_walk_agree(chains):
    (ta, da, X, _), (tb, db, Xb, _) = chains["4095"], chains["4097"]
    a, b = run_tree(ta, X), run_tree(tb, X)  # the same rows through both
    shared = X[:, 0] < da  # both chains end these at leaf 2 d + 1
    assert shared.sum() > 200 and np.array_equal(a.leaf[shared], b.leaf[shared]) and np.array_equal(a.pred[shared], b.pred[shared])
    assert np.all(a.leaf[~shared] == 2 * da) and np.all(np.isin(b.leaf[~shared], (2 * da + 1, 2 * db)))
    assert a.bad == 0 and b.bad == 0


def test_tree_row_count_and_row_value_edges(chains):
    """Nq = 0, 1, 255, 256, 257 on the 4096-node table; then NaN, +-inf, the midpoint between FLT_MAX and
    2^128 and its negative in either column, in the last lane of a workgroup and the row after it:
    unanswered and counted; the double just under the midpoint is FLT_MAX as float32 and is answered."""
    t, depth, X, (want, _) = chains["4096"]
    for n in E.TREE_QUERY_COUNTS:
        r = check_tree(t, X[:n], want[:n])
        assert len(r.pred) == n and r.bad == 0
    Xb = X.copy()
    cells = [(0, 0, np.nan), (255, 1, np.inf), (256, 0, -np.inf), (100, 1, E.MIDPOINT), (101, 0, -E.MIDPOINT),
             (102, 1, float(np.nextafter(E.MIDPOINT, np.inf)))]
    for r_, c_, v in cells:
        Xb[r_, c_] = v
    Xb[103, 1] = float(np.nextafter(E.MIDPOINT, 0.0))
    wb = R.tree_walk(t, Xb)[1]
    bad = np.array([r_ for r_, _, _ in cells])
    assert np.all(wb[bad] == -1) and (wb < 0).sum() == len(bad) and wb[103] >= 0
    r = check_tree(t, Xb, wb)
    assert r.bad == len(bad)


@pytest.mark.parametrize("thr", E.THRESHOLDS, ids=repr)
def test_tree_threshold_edges(thr):
    """A stump per threshold edge (+-0, the smallest float32 subnormal and half of it, subnormals between two
    float32s, +-1e-50, FLT_MAX and the doubles next to it, +-1e40, +-inf; NaN: every comparison is false, the
    walk goes right), asked at the threshold, a float32 ulp either side, the doubles that round onto it,
    +-1e-46 and the rounding midpoint to overflow with its neighbours."""
    vals = E.stump_values(thr)
    want = E.stump_leaf(thr, vals)
    t = E.stump(thr)
    assert np.array_equal(R.tree_walk(t, vals[:, None])[1], want)
    r = check_tree(t, vals[:, None], want)
    print(repr(thr), r.leaf.tolist())


@pytest.mark.parametrize("seed", [1, 2])
def test_tree_fitted_on_subnormal_data(seed):
    """scikit-learn's own trees with float32-subnormal thresholds: its apply and predict, row for row (a
    flushed subnormal would change decisions)."""
    tree, Q = E.subnormal_tree(seed)
    t = R.tree_arrays(tree)
    r = check_tree(t, Q, tree.apply(Q))
    assert r.bad == 0 and np.array_equal(t["classes"][r.pred], tree.predict(Q))
    clf = _classifier('decision_tree', tree)
    assert np.array_equal(clf.predict(Q), tree.predict(Q)) and np.array_equal(clf.apply(Q), tree.apply(Q))
    assert clf.last_predict_stats == {'device': True, 'uncertified': 0}
    Qb = Q.copy()
    Qb[4, 1] = np.nan  # scikit-learn's missing value: its own answer
    assert same_outcome(clf.predict, tree.predict, Qb) and same_outcome(clf.apply, tree.apply, Qb)
    assert clf.last_predict_stats == {'device': True, 'uncertified': 1}
    for v in (np.inf, -np.inf, E.MIDPOINT, 1e39):  # not finite as float32: its own exception
        Qb[9, 2] = v
        with pytest.raises(ValueError):
            tree.predict(Qb)
        for ours, theirs in ((clf.predict, tree.predict), (clf.apply, tree.apply)):
            assert same_outcome(ours, theirs, Qb) and _outcome(ours, Qb)[0] == "raises"
            assert clf.last_predict_stats == {'device': True, 'uncertified': 2}


@pytest.mark.parametrize("D", [1, 4096])
def test_tree_one_column_and_the_widest_row(D):
    """D = 1, and D = 4096 with the tested feature last: every column is checked for a value that is not finite
    as float32, the first and the last included."""
    rng = np.random.default_rng(D)
    X = rng.normal(0.0, 1.0, (257, D))
    bad = {5: (0, np.nan), 6: (D - 1, 1e39), 256: (D // 2, np.inf), 255: (D - 1, E.MIDPOINT)}
    for r_, (c_, v) in bad.items():
        X[r_, c_] = v
    t = E.stump(0.25, D=D, feature=D - 1)
    want = E.stump_leaf(0.25, X[:, D - 1])
    want[list(bad)] = -1
    assert np.array_equal(R.tree_walk(t, X)[1], want) and {1, 2, -1} == set(want.tolist())
    check_tree(t, X, want)


@pytest.mark.parametrize("kw", [dict(D=0), dict(D=4097), dict(n_nodes=0), dict(max_depth=-1), dict(Nq=-1),
                                dict(null="left"), dict(null="threshold"), dict(null="leaf_class"), dict(short=1)], ids=str)
def test_tree_rejected_arguments_touch_nothing(kw):
    from src import _hip
    t = E.chain_tree(9)
    L = TreeLaunch(t, E.chain_queries(4, 7), **kw)
    assert L.call() == (_hip.DSP_ERR_WORKSPACE if "short" in kw else _hip.DSP_ERR_ARGS)
    assert L.untouched() and L.counter() == int.from_bytes(bytes([JUNK] * 4), "little")


# ---- graph capture ---------------------------------------------------------------------------------------
def _replay_twice(L, eager, same):
    """One call captured on a single stream (no parallel branches), replayed twice over outputs refilled with
    the sentinel and a counter refilled with garbage: the eager results, and the counter reads 2."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert L.call() == 0
    for _ in range(2):
        L.refill()
        graph.replay()
        r = L.read()
        same(r, eager)
        assert L.counter() == 2


def test_nb_graph_replay_resets_the_counter():
    _, m = E.fitted(10, 40)
    ties = E.banded_queries(m, (3, 7))[0][8:10]  # the two doubles either side of a tie: uncertifiable
    X = E.queries(m, 60, 21)
    X = np.concatenate([X[:40], ties, X[40:]])
    L = NbLaunch(m, X)
    assert L.call() == 0
    eager = L.read()
    assert eager.unc == 2 and np.flatnonzero(eager.cert == 0).tolist() == [40, 41]

    def same(r, e):
        assert same_bits(r.jll, e.jll) and np.array_equal(r.pred, e.pred) and np.array_equal(r.cert, e.cert)
    _replay_twice(L, eager, same)


def test_tree_graph_replay_resets_the_counter(chains):
    t, depth, X, _ = chains["4095"]
    X = X[:62].copy()
    X[40, 0], X[41, 1] = np.nan, E.MIDPOINT  # unanswerable
    L = TreeLaunch(t, X)
    assert L.call() == 0
    eager = L.read()
    assert eager.bad == 2 and np.flatnonzero(eager.leaf < 0).tolist() == [40, 41]
    assert np.array_equal(eager.leaf, R.tree_walk(t, X)[1])

    def same(r, e):
        assert np.array_equal(r.leaf, e.leaf) and np.array_equal(r.pred, e.pred)
    _replay_twice(L, eager, same)
