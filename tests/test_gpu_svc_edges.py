"""dsp_svc_predict (csrc/svm.hip) at its shape and numeric edges (tests/svc_edge_cases.py), through the
bare C ABI: 64 NaNs stand behind sv, dual_coef, intercept and the queries and 1 << 20 behind n_support, so
a read past an array shows in dec; pred, dec and certified lie between guard rows (tests/device_outputs.py).

The tolerance is the project's derived bound (tests/svc_reference.dec_bound) against the
exact decimal value (svc_edge_cases.exact_dec) on the rows svc_edge_cases.exact_rows picks, and against
the numpy restatement -- a second fp64 evaluation, which the bound is about -- on the others.  Every
check prints its largest err / bound."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import svc_edge_cases as E
import svc_reference as R
from conftest import GOLDEN
from device_outputs import Guarded, bits

pytestmark = pytest.mark.gpu

FILL = -5
TAIL = 64


def _behind(a, np_dtype, tail):
    a = np.asarray(a, np_dtype).ravel()
    return torch.as_tensor(np.concatenate([a, np.full(TAIL, tail, np_dtype)])).to("cuda")


class Launch:
    """One dsp_svc_predict call's buffers.  The keyword arguments replace what the model says."""

    def __init__(self, m, X, with_dec=True, n_support=None, gamma=None, D=None, C=None, short=0):
        from src import _hip
        self.lib, self.hip = _hip.lib(), _hip
        X = np.ascontiguousarray(X, np.float64)
        self.nSV, d = m['sv'].shape
        c = len(m['n_support'])
        self.Nq, self.P = X.shape[0], c * (c - 1) // 2
        self.D, self.C = d if D is None else D, c if C is None else C
        self.gamma = float(m['gamma'] if gamma is None else gamma)
        self.shape = (self.nSV, self.Nq, d, c)
        nbytes = self.lib.dsp_svc_workspace_bytes(*self.shape)
        assert nbytes > 0
        self.nbytes = nbytes - short
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        self.sv = _behind(m['sv'], np.float64, np.nan)
        self.ns = _behind(m['n_support'] if n_support is None else n_support, np.int32, 1 << 20)
        self.coef = _behind(m['dual_coef'], np.float64, np.nan)
        self.b = _behind(m['intercept'], np.float64, np.nan)
        self.q = _behind(X, np.float64, np.nan)
        self.pred = Guarded((self.Nq,), torch.int32, FILL)
        self.cert = Guarded((self.Nq,), torch.int32, FILL)
        self.dec = Guarded((self.Nq, self.P), torch.float64, float(FILL)) if with_dec else None
        self.off = self.lib.dsp_svc_workspace_uncertified_offset(*self.shape)

    def call(self):
        p = self.hip.ptr
        return self.lib.dsp_svc_predict(p(self.sv), p(self.ns), p(self.coef), p(self.b), self.nSV, self.D, self.C,
                                        self.gamma, p(self.q), self.Nq, p(self.pred.view),
                                        p(self.dec.view) if self.dec else None, p(self.cert.view), p(self.ws),
                                        self.nbytes, self.hip.stream_handle())

    def refill(self):
        for o in (self.pred, self.cert, self.dec):
            if o is not None:
                o.view.fill_(FILL)

    def read(self):
        """(the guards are checked by Guarded.get)"""
        torch.cuda.synchronize()
        return SimpleNamespace(pred=self.pred.get(), cert=self.cert.get(), dec=self.dec.get() if self.dec else None,
                               unc=int(self.ws[self.off:self.off + 4].view(torch.int32).item()))

    def untouched(self):
        r = self.read()
        return all(np.all(a == FILL) for a in (r.pred, r.cert, r.dec) if a is not None)


def run(m, X, **kw):
    L = Launch(m, X, **kw)
    rc = L.call()
    assert rc == 0, rc
    return L.read()


def reference(m, X):
    """(dec [Nq, P], bound [Nq, P]): exact on exact_rows, the restatement's elsewhere; computed once per
    use and sliced by the tests that launch a part of X."""
    with np.errstate(over='ignore'):
        ref, bound = R.decision_values(m, X), R.dec_bound(m, X)
    rows = E.exact_rows(m, len(X))
    ref[rows] = E.exact_dec(m, X[rows])[1]
    return ref, bound


def check(tag, m, r, ref, bound):
    """dec within the bound; counter and flags agree; a certified row's vote is the reference's."""
    err = np.abs(r.dec - ref)
    worst = (err / bound).max()
    print("%s: max err / bound %.3g, certified %d of %d" % (tag, worst, int(r.cert.sum()), len(r.cert)))
    assert not np.isnan(r.dec).any(), "a read past an input array"
    assert np.all(err <= bound), worst
    assert set(np.unique(r.cert)) <= {0, 1} and r.unc == int((r.cert == 0).sum())
    C = len(m['n_support'])
    assert r.pred.min() >= 0 and r.pred.max() < C
    won = r.cert == 1
    assert np.array_equal(r.pred[won], R.vote(ref, C)[won])
    assert np.all(np.abs(ref[won]) > (R.SAFETY - 1.0) * bound[won])  # a certificate is never given inside 3 bounds
    return worst


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- shapes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", E.CLASS_COUNTS)
def test_class_count_edges(C):
    """Either side of every svc_main<DP, CR>: a padded coefficient row is or is not the last live one."""
    m = E.class_count_model(C)
    X = E.queries(m, E.EDGE_NQ, C)
    check("C=%d" % C, m, run(m, X), *reference(m, X))


@pytest.mark.parametrize("C,D", [(3, D) for D in E.DIMS] + list(E.CORNERS))
def test_dimension_edges(C, D):
    """Either side of DP = 16 | 32 | chunks, a whole number of chunks, the plan's limit; Nq = 130 and 5."""
    m = E.dim_model(D) if C == 3 else E.class_count_model(C, D)
    X = E.queries(m, E.EDGE_NQ, D)
    ref, bound = reference(m, X)
    many, few = run(m, X), run(m, X[:5])
    check("C=%d D=%d Nq=130" % (C, D), m, many, ref, bound)
    check("C=%d D=%d Nq=5" % (C, D), m, few, ref[:5], bound[:5])
    assert same_bits(many.dec[:5], few.dec[:5]) and np.array_equal(many.pred[:5], few.pred[:5])


def test_query_count_edges():
    """Around the 128-query workgroup and the 512-query end of the SV-split launch: row 0 keeps its bits
    at every count and as the last row (the one idle lanes shadow)."""
    from src import _hip
    m = E.query_count_model()
    X = E.queries(m, max(E.QUERY_COUNTS), 1)
    ref, bound = reference(m, X)
    parts = {n: _hip.lib().dsp_svc_launch_parts(600, n, 5, 3) for n in E.QUERY_COUNTS}
    assert parts[512] == 3 and parts[513] == 1, parts  # 512 ran split, 513 ran tiled
    row0 = None
    for n in E.QUERY_COUNTS:
        r = run(m, X[:n])
        check("Nq=%d" % n, m, r, ref[:n], bound[:n])
        row0 = r if row0 is None else row0
        assert same_bits(r.dec[0], row0.dec[0]) and r.pred[0] == row0.pred[0] and r.cert[0] == row0.cert[0], n
        moved = run(m, np.concatenate([X[1:n], X[:1]]))
        assert same_bits(moved.dec[-1], row0.dec[0]) and moved.pred[-1] == row0.pred[0], n
        assert same_bits(moved.dec[:-1], r.dec[1:])


def test_split_byte_cap():
    """C = 64, nSV = 1025: 416 queries run in 5 parts, 417 in one (64 MiB of parts); same bits."""
    from src import _hip
    m = E.byte_cap_model()
    lo, hi = E.BYTE_CAP_NQ
    assert [_hip.lib().dsp_svc_launch_parts(1025, n, 2, 64) for n in (lo, hi)] == [5, 1]
    X = E.queries(m, hi, 2)
    ref, bound = reference(m, X)
    a, b = run(m, X[:lo]), run(m, X)
    check("byte cap Nq=%d" % lo, m, a, ref[:lo], bound[:lo])
    check("byte cap Nq=%d" % hi, m, b, ref, bound)
    assert same_bits(a.dec, b.dec[:lo]) and np.array_equal(a.pred, b.pred[:lo]) and np.array_equal(a.cert, b.cert[:lo])


@pytest.mark.parametrize("name", list(E.segment_models()))
def test_segments_and_tiles(name):
    """Classes of 0, 1, 31, 32, 33 and 300 rows in three segments (the one-row class leaves two empty),
    on the 32-row and the 16-row tile; nSV on either side of one segment | two."""
    m = E.segment_models()[name]
    X = E.queries(m, E.EDGE_NQ, 3)
    ref, bound = reference(m, X)
    many, few = run(m, X), run(m, X[:5])
    check(name + " Nq=130", m, many, ref, bound)
    check(name + " Nq=5", m, few, ref[:5], bound[:5])
    assert same_bits(many.dec[:5], few.dec[:5])


def test_segment_clamp():
    """nSV = 16 385: 65 segments clamped to 64, a one-row class with 63 empty ones; 64 parts at Nq = 5, one
    at 600, the first five rows alike; rows 0, 2 and 4 against the exact value."""
    from src import _hip
    m = E.large_model()
    assert [_hip.lib().dsp_svc_launch_parts(16385, n, 2, 3) for n in (5, 600)] == [64, 1]
    X = E.queries(m, 600, 8)
    ref, bound = R.decision_values(m, X), R.dec_bound(m, X)
    ref[[0, 2, 4]] = E.exact_dec(m, X[[0, 2, 4]])[1]
    few, many = run(m, X[:5]), run(m, X)
    check("nSV=16385 Nq=5", m, few, ref[:5], bound[:5])
    check("nSV=16385 Nq=600", m, many, ref, bound)
    assert same_bits(few.dec, many.dec[:5]) and np.array_equal(few.pred, many.pred[:5])


# ---- arguments -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(D=4097), dict(C=1), dict(C=65), dict(gamma=-1.0), dict(gamma=float("nan")),
                                dict(short=1)], ids=str)
def test_rejected_arguments_touch_nothing(kw):
    m = E.dim_model(15)
    L = Launch(m, E.queries(m, 7, 4), **kw)
    assert L.call() != 0
    assert L.untouched()


def test_dec_null():
    m = E.segment_models()["tiles"]
    X = E.queries(m, E.EDGE_NQ, 5)
    a, b = run(m, X), run(m, X, with_dec=False)
    assert b.dec is None and np.array_equal(a.pred, b.pred) and np.array_equal(a.cert, b.cert) and a.unc == b.unc


@pytest.mark.parametrize("change", [-50, 50, "negative"])
@pytest.mark.parametrize("name", ["tiles", "tiles_hd"])
def test_malformed_n_support_stays_inside_the_arrays(name, change):
    """A sum below nSV, a sum above it, a negative entry: svc_segment clamps every row range into
    [0, nSV), so the call returns 0, no NaN from behind the arrays reaches dec and the guards stand."""
    m = E.segment_models()[name]
    ns = m['n_support'].copy()
    if change == "negative":
        ns[2] = -40
    else:
        ns[5] += change
    r = run(m, E.queries(m, E.EDGE_NQ, 6), n_support=ns)
    assert not np.isnan(r.dec).any()
    assert r.unc == int((r.cert == 0).sum()) and r.pred.min() >= 0 and r.pred.max() < len(ns)


# ---- numeric edges ---------------------------------------------------------------------------------
def test_kernel_value_edges():
    """K = 1 exactly, subnormal, 0 by underflow and 0 by an overflowing d^2, on a fitted model."""
    sk, m, _ = E.fitted(3, 4)
    nq = E.numeric_queries(m)
    names = ("on_sv", "subnormal", "underflow", "huge")
    X = np.concatenate([nq[n] for n in names] + [E.queries(m, 20, 9)])
    r = run(m, X)
    check("kernel values", m, r, *reference(m, X))
    zero = slice(4, 11)  # underflow and huge: dec is the intercept, bit for bit
    assert same_bits(r.dec[zero], np.tile(m['intercept'], (7, 1)))
    assert np.array_equal(m['classes'][r.pred[zero]], sk.predict(X[zero]))
    assert np.array_equal(m['classes'][r.pred[r.cert == 1]], sk.predict(X)[r.cert == 1])


def test_zero_intercept_is_a_tie():
    sk, m, _ = E.fitted(3, 4)
    b = m['intercept'].copy()
    b[1] = 0.0
    z = E.variant(m, "b1=0", intercept=b)
    X = np.concatenate([E.numeric_queries(m)["underflow"], E.queries(m, 4, 10)])
    r = run(z, X)
    check("zero intercept", z, r, *reference(z, X))
    assert bits(r.dec[0, 1]) == 0 and r.cert[0] == 0 and r.unc >= 1
    want = R.vote(np.array([b]), 3)[0]  # pair (0, 2) at dec = 0 votes for class 2
    assert r.pred[0] == want


@pytest.mark.parametrize("gamma", [0.0, 1e-300, 1e300])
def test_gamma_ends(gamma):
    _, m, _ = E.fitted(3, 4)
    g = E.variant(m, "gamma=%g" % gamma, gamma=np.float64(gamma))
    X = np.concatenate([E.numeric_queries(m)["on_sv"], E.queries(m, 12, 11)])
    check("gamma=%g" % gamma, g, run(g, X), *reference(g, X))


def test_gamma_inf():
    """gamma >= 0 admits +inf: K = 0 for every d^2 > 0, and inf * 0 = NaN for a query equal to a support vector."""
    _, m, _ = E.fitted(3, 4)
    X = np.concatenate([E.queries(m, 8, 12), E.numeric_queries(m)["on_sv"]])
    r = run(m, X, gamma=float("inf"))
    assert same_bits(r.dec[:8], np.tile(m['intercept'], (8, 1)))
    assert np.all(r.cert[8:] == 0) and np.all(np.isnan(r.dec[8:]).any(axis=1))
    assert r.unc == int((r.cert == 0).sum())


def test_coefficient_ends():
    """All-zero coefficients (A = 0: dec = b, certified since b != 0), one zero column, +-1e300 (no sum of
    K <= 1 terms overflows: finite, within the bound) and +-1.7e308 (sums overflow: inf or NaN in dec, and
    B_q or A is inf, so no row is certified)."""
    _, m, _ = E.fitted(3, 4)
    X = np.concatenate([E.numeric_queries(m)["on_sv"], E.numeric_queries(m)["underflow"], E.queries(m, 12, 13)])
    zero = E.variant(m, "coef=0", dual_coef=np.zeros_like(m['dual_coef']))
    r = run(zero, X)
    assert np.all(m['intercept'] != 0)
    assert same_bits(r.dec, np.tile(m['intercept'], (len(X), 1))) and np.all(r.cert == 1) and r.unc == 0
    assert np.array_equal(r.pred, R.vote(r.dec, 3))
    coef = m['dual_coef'].copy()
    coef[:, 5] = 0.0
    col = E.variant(m, "col5=0", dual_coef=coef)
    check("zero column", col, run(col, X), *reference(col, X))
    big = E.variant(m, "coef=1e300", dual_coef=np.sign(m['dual_coef']) * 1e300)
    r = run(big, X)
    check("coef 1e300", big, r, *reference(big, X))
    top = E.variant(m, "coef=1.7e308", dual_coef=np.sign(m['dual_coef']) * 1.7e308)
    r = run(top, X)
    assert (~np.isfinite(r.dec)).any() and np.all(r.cert == 0) and r.unc == len(X)


# ---- rows that are not finite ----------------------------------------------------------------------
def nonfinite_cases():
    """(name, model, [(row, column)]) at Nq = 129: the first and the last column, a column of a later
    chunk, and row 128 -- alone in its workgroup, the row its idle lanes shadow."""
    hd = E.segment_models()["tiles_hd"]  # D = 40, three parts
    return [("d4", E.fitted(3, 4)[1], [(3, 0), (70, 3), (128, 1)]),
            ("d17", E.dim_model(17), [(0, 0), (127, 16), (128, 16)]),
            ("d40", hd, [(5, 0), (64, 16), (100, 39), (128, 23)])]


@pytest.mark.parametrize("bad", E.NONFINITE, ids=str)
@pytest.mark.parametrize("case", nonfinite_cases(), ids=lambda c: c[0])
def test_rows_that_are_not_finite_are_uncertified(case, bad):
    name, m, cells = case
    X = E.queries(m, 129, 14)
    clean = run(m, X)
    assert clean.unc == 0
    Xb = X.copy()
    for r_, c_ in cells:
        Xb[r_, c_] = bad
    rows = np.array([r_ for r_, _ in cells])
    r = run(m, Xb)
    assert np.all(r.cert[rows] == 0) and r.unc == len(rows)
    assert np.all(np.isnan(r.dec[rows]))
    keep = np.setdiff1d(np.arange(129), rows)
    assert same_bits(r.dec[keep], clean.dec[keep]) and np.array_equal(r.pred[keep], clean.pred[keep])
    assert np.all(r.cert[keep] == 1)


def test_classifier_raises_where_scikit_learn_does():
    from src.models import TraditionalClassifier
    sk, m, Xtr = E.fitted(3, 4)
    clf = TraditionalClassifier('svm', C=1.0, kernel='rbf')
    clf.model = sk
    for bad in E.NONFINITE:
        X = Xtr[:50].copy()
        X[7, 0] = X[20, 3] = X[49, 2] = bad
        for ours, theirs in ((clf.predict, sk.predict), (clf.decision_function, sk.decision_function)):
            with pytest.raises(ValueError):
                theirs(X)
            clf.last_predict_stats = None
            with pytest.raises(ValueError):
                ours(X)
            assert clf.last_predict_stats == {'device': True, 'uncertified': 3}
    X = np.concatenate([Xtr[:50], E.numeric_queries(m)["huge"]])  # huge but finite: neither refuses
    assert np.array_equal(clf.predict(X), sk.predict(X))
    assert clf.last_predict_stats == {'device': True, 'uncertified': 0}
    dec = clf.decision_function(X)
    assert np.all(np.abs(dec - sk.decision_function(X)) <= reference(m, X)[1])


# ---- the certificate -------------------------------------------------------------------------------
BAND_TOL = 0.05  # the host test holds every banded query within this of its target


@pytest.mark.parametrize("C,D,p", [(2, 4, 0), (3, 4, 0), (3, 4, 1), (3, 4, 2), (11, 6, 7)])
def test_certificate_threshold(C, D, p):
    """Queries 0 .. 1000 bounds from a tie of pair p, every other pair decided.  The device's dec is within
    one bound of the exact value and it certifies above SVC_SAFETY = 4 of its own bound, so a row at
    most 2.4 bounds out (the tolerance of the targets included) must not be certified and a row 6.2 or
    more out must be; no row is left out, and a certified vote is libsvm's."""
    sk, m, _ = E.fitted(C, D)
    X, ratio = E.banded_queries(m, p)
    exact, bound = E.exact_dec(m, X)[1], R.dec_bound(m, X)
    r = run(m, X)
    err = np.abs(r.dec - exact) / bound
    print("C=%d pair %d: exact / bound %s, certified %s, max err / bound %.3g"
          % (C, p, np.round(ratio, 3).tolist(), r.cert.tolist(), err.max()))
    assert np.all(err <= 1.0), err.max()
    inside, outside = np.abs(ratio) <= E.MUST_NOT + BAND_TOL, np.abs(ratio) >= E.MUST - BAND_TOL
    assert inside.sum() == 4 and outside.sum() == 4  # all eight rows stand under one of the two rules
    assert np.all(r.cert[inside] == 0), (ratio, r.cert)
    assert np.all(r.cert[outside] == 1), (ratio, r.cert)
    assert r.unc == 4
    won = r.cert == 1
    assert np.array_equal(r.pred[won], R.vote(exact, C)[won])
    assert np.array_equal(m['classes'][r.pred[won]], sk.predict(X)[won])


# ---- graph capture ---------------------------------------------------------------------------------
def test_graph_replay_resets_the_counter():
    """One call captured, replayed twice over outputs filled with -5: the eager bits, and the uncertified
    counter reads 2 after each replay -- its memset is part of the graph."""
    g = np.load(os.path.join(GOLDEN, "svc_golden.npz"))
    m = {k: g["c10/" + k] for k in ("sv", "n_support", "dual_coef", "intercept", "gamma", "classes")}
    X = np.concatenate([g["c10/X"][:40], g["c10/tie_X"], g["c10/X"][40:60]])
    L = Launch(m, X)
    assert L.call() == 0
    eager = L.read()
    assert eager.unc == 2 and np.flatnonzero(eager.cert == 0).tolist() == [40, 41]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert L.call() == 0
    for _ in range(2):
        L.refill()
        graph.replay()
        r = L.read()
        assert same_bits(r.dec, eager.dec) and np.array_equal(r.pred, eager.pred) and np.array_equal(r.cert, eager.cert)
        assert r.unc == 2
