"""Edge cases of SVC prediction (csrc/svm.hip, dsp_svc_predict): the exact value of the contract, models
built by hand at every class count, dimension, support-vector count and class size where the kernel
or its launch plan takes another path, queries placed a chosen number of bounds from a tie, and the
numeric ends of exp(-gamma d^2) (a plain helper module like tests/knn_edge_cases.py: no test, no
fixture; it never touches the device library).  tests/test_svc_edges_host.py pins on the CPU that
every case hits what it claims; tests/test_gpu_svc_edges.py runs them.

Models are dicts in tests/svc_reference.py's form with a ``name`` (the key of the exact values' cache).
"""
import decimal

import numpy as np

import svc_reference as R

PREC = 60                 # decimal digits of exact_dec
EXACT_BUDGET = 100_000    # support-vector elements (nSV x D x rows) a check spends on exact_dec ...
EXACT_MIN_ROWS = 3        # ... but never fewer rows than this
_CTX = decimal.Context(prec=PREC, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)
_EXACT = {}
_SV_DEC = {}


def _dec_rows(a):
    return [[decimal.Decimal(float(v)) for v in row] for row in np.asarray(a, np.float64)]


def exact_dec(model, X):
    """The contract of include/dsp_audiorec.h in decimal arithmetic at 60 digits: Decimal(float) is
    exact, sums and products of so few terms are exact or rounded at 1e-60, Decimal.exp() is correctly
    rounded.  Returns (decimals [Nq][P], their nearest doubles [Nq, P]).  An exp whose argument is below
    -2.4e6 is 0: that is under 1e-1000000, less than a decimal of this context can hold.  Rows are
    finite; gamma is finite."""
    X = np.atleast_2d(np.asarray(X, np.float64))
    key = model['name']
    if key not in _SV_DEC:
        _SV_DEC[key] = (_dec_rows(model['sv']), _dec_rows(model['dual_coef']),
                        [decimal.Decimal(float(v)) for v in model['intercept']], decimal.Decimal(float(model['gamma'])))
    sv, coef, b, gamma = _SV_DEC[key]
    ns = [int(n) for n in model['n_support']]
    start = np.concatenate([[0], np.cumsum(ns)]).tolist()
    C = len(ns)
    pr = R.pairs(C)
    out = []
    ctx, zero = _CTX, decimal.Decimal(0)
    for row in X:
        ck = (key, row.tobytes())
        if ck not in _EXACT:
            q = [decimal.Decimal(float(v)) for v in row]
            K = []
            for s in sv:
                d2 = zero
                for a, c in zip(q, s):
                    t = ctx.subtract(a, c)
                    d2 = ctx.fma(t, t, d2)
                x = ctx.multiply(gamma, d2)
                K.append(zero if x > 2400000 else ctx.exp(ctx.minus(x)))
            dec = []
            for p, (i, j) in enumerate(pr):
                v = b[p]
                for s in range(start[i], start[i + 1]):
                    v = ctx.fma(coef[j - 1][s], K[s], v)
                for s in range(start[j], start[j + 1]):
                    v = ctx.fma(coef[i][s], K[s], v)
                dec.append(v)
            _EXACT[ck] = dec
        out.append(_EXACT[ck])
    return out, np.array([[float(v) for v in r] for r in out], np.float64).reshape(len(out), len(pr))


def exact_rows(model, Nq):
    """The rows a check spends exact_dec on: all of them while nSV x D x Nq stays inside EXACT_BUDGET,
    else EXACT_BUDGET's worth (at least EXACT_MIN_ROWS) spread from the first row to the last; the
    other rows are compared with the numpy restatement, within the same bound."""
    per_row = model['sv'].size
    n = max(EXACT_MIN_ROWS, EXACT_BUDGET // max(per_row, 1))
    if n >= Nq:
        return np.arange(Nq)
    return np.unique(np.linspace(0, Nq - 1, n).round().astype(np.int64))


def hand_model(C, D, n_support, seed, gamma=None, name=None):
    """A model built directly, not fitted: normal support vectors, dual coefficients and intercepts,
    gamma = 1 / (D var) (scikit-learn's 'scale') unless given, labels 1, 4, 7, ..."""
    n_support = np.asarray(n_support, np.int32)
    assert n_support.shape == (C,) and n_support.min() >= 0
    nSV = int(n_support.sum())
    rng = np.random.default_rng(seed)
    sv = rng.normal(0.0, 1.0, (nSV, D))
    coef = rng.normal(0.0, 1.0, (C - 1, nSV))
    b = rng.normal(0.0, 0.5, C * (C - 1) // 2)
    if gamma is None:
        gamma = 1.0 / (D * sv.var())
    return dict(sv=sv, n_support=n_support, dual_coef=coef, intercept=b, gamma=np.float64(gamma),
                classes=np.arange(C) * 3 + 1, name=name or "hand-%d-%d-%d-%d" % (C, D, nSV, seed))


def variant(model, name, **changes):
    """A copy of ``model`` with some arrays replaced (its own name: its own exact values)."""
    m = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in model.items()}
    m.update(changes)
    m['name'] = model['name'] + "/" + name
    return m


def queries(model, Nq, seed):
    """Nq rows near the support vectors: kernel values of every size, dec of both signs."""
    rng = np.random.default_rng(seed)
    sv = model['sv']
    return sv[rng.integers(0, sv.shape[0], Nq)] + rng.normal(0.0, 0.7, (Nq, sv.shape[1]))


# ---- shapes ------------------------------------------------------------------------------------
# svc_main<DP, CR>: CR = 1, 3, 9, 31, 63 at C <= 2, 4, 10, 32 and above; each C on either side
CLASS_COUNTS = (2, 3, 4, 5, 10, 11, 32, 33, 64)
# DP = 16, 32 and chunks of 16: D on either side, an exact multiple of the chunk, the plan's limit
DIMS = (1, 15, 16, 17, 32, 33, 48, 4096)
CORNERS = ((33, 33), (64, 17))
# SVC_T = 128 queries per workgroup; the SV-split launch up to 512 queries
QUERY_COUNTS = (1, 127, 128, 129, 256, 257, 512, 513)
EDGE_NQ = 130  # two workgroups, the second with 2 live lanes


def _six_and_a_one(C):
    ns = np.full(C, 6, np.int32)
    ns[C // 2] = 1
    return ns


def class_count_model(C, D=3):
    """About six rows per class, one class of one row."""
    return hand_model(C, D, _six_and_a_one(C), 100 + C + 1000 * D)


def dim_model(D):
    """Classes of 15, 16 and 9 rows: one row under a tile of the D > 32 path, a whole tile, and less."""
    return hand_model(3, D, [15, 16, 9], 200 + D)


def query_count_model():
    """nSV = 600: G = 3 segments, split for Nq <= 512."""
    return hand_model(3, 5, [200, 250, 150], 300)


BYTE_CAP_NQ = (416, 417)  # 64 x 63 x Nq x 8 x 5 bytes is 64 MiB - 40 KiB at 416 and above 64 MiB at 417


def byte_cap_model():
    """C = 64, nSV = 1025 (G = 5): the parts of the SV-split launch reach its byte cap before Nq = 512."""
    ns = np.full(64, 16, np.int32)
    ns[0] = 17
    return hand_model(64, 2, ns, 301)


TILE_CLASSES = (0, 1, 31, 32, 33, 300, 120)  # nSV = 517, G = 3: the one-row class has two empty segments


def segment_models():
    """name -> model: class sizes on the 32-row tile edge with G >= 3, and nSV on either side of G = 1 | 2."""
    return {"tiles": hand_model(len(TILE_CLASSES), 4, TILE_CLASSES, 400),
            "tiles_hd": hand_model(len(TILE_CLASSES), 40, TILE_CLASSES, 401),
            "nsv256": hand_model(3, 4, [100, 100, 56], 402),
            "nsv257": hand_model(3, 4, [100, 100, 57], 403)}


def large_model():
    """nSV = 16 385: ceil(nSV / 256) = 65 segments clamped to 64; a class of one row with 63 empty segments."""
    return hand_model(3, 2, [1, 16000, 384], 404)


# ---- fitted models ---------------------------------------------------------------------------------
_FITTED = {}


def fitted(C, D, per_class=40, seed=0):
    """(the scikit-learn SVC, its arrays): C overlapping Gaussian classes, fitted once per shape."""
    key = (C, D, per_class, seed)
    if key not in _FITTED:
        from sklearn.svm import SVC
        rng = np.random.default_rng(500 + 31 * C + D + seed)
        centres = rng.normal(0.0, 1.2, (C, D))
        X = np.concatenate([c + rng.normal(0.0, 1.0, (per_class, D)) for c in centres])
        y = np.repeat(np.arange(C) * 2 + 3, per_class)
        sk = SVC(C=1.0, kernel='rbf', random_state=42).fit(X, y)
        sk.decision_function_shape = 'ovo'
        m = R.model_arrays(sk)
        m['name'] = "fitted-%d-%d-%d-%d" % key
        _FITTED[key] = (sk, m, X)
    return _FITTED[key]


# ---- numeric edges ---------------------------------------------------------------------------------
def numeric_queries(model):
    """name -> rows [n, D] of a model's numeric edge queries:
      on_sv       three support vectors themselves (K = 1 exactly for their own row)
      subnormal   support vector 0 moved by sqrt(720 / gamma) along the first axis: gamma d^2 = 720 for it,
                  exp(-720) = 2e-313 is subnormal
      underflow   beyond every support vector by sqrt(800 / gamma) along the first axis: every K is 0
      huge        1e160 and 1.7e308 (and their negatives) in the first, the last or every column:
                  d^2 overflows to inf, every K is 0"""
    sv, g = model['sv'], float(model['gamma'])
    D = sv.shape[1]
    sub = sv[0].copy()
    sub[0] += np.sqrt(720.0 / g)
    far = sv.mean(axis=0)
    far[0] = sv[:, 0].max() + np.sqrt(800.0 / g)
    huge = np.tile(sv.mean(axis=0), (6, 1))
    huge[0, 0] = 1e160
    huge[1, D - 1] = -1e160
    huge[2, 0] = 1.7e308
    huge[3, D - 1] = -1.7e308
    huge[4, :] = 1.7e308
    huge[5, :] = -1e160
    return {"on_sv": sv[[0, sv.shape[0] // 2, sv.shape[0] - 1]].copy(), "subnormal": sub[None, :],
            "underflow": far[None, :], "huge": huge}


NONFINITE = (np.inf, -np.inf, np.nan)


# ---- the certificate's threshold -------------------------------------------------------------------
BAND_KS = (0.0, 0.5, 2.0, 2.4, 6.2, 8.0, 30.0, 1000.0)
MUST_NOT = 2.4   # |dec_exact| <= 2.4 bound: the device's dec is within one bound of it, so at most
                 # 3.4 bound < SVC_SAFETY bound -- must not be certified
MUST = 6.2       # |dec_exact| >= 6.2 bound: the device's dec is at least 5.2 bound, and its own bound
                 # (from its B_q, within rounding of the restatement's) is passed with room -- must be
OTHER_PAIRS = 6.2


def banded_queries(model, p, ks=BAND_KS, seed=0):
    """(X [len(ks), D], ratio [len(ks)]): queries on a segment between two rows of opposite dec_p sign at
    which the numpy restatement's dec_p - k bound_p crosses zero, one per k, and dec_exact / bound of
    pair p at each.  Every other pair of every returned query is at |dec_exact| >= OTHER_PAIRS bound
    (asserted), so pair p alone decides the certificate."""
    rng = np.random.default_rng(9000 + 17 * p + seed)
    sv = model['sv']
    cand = sv[rng.integers(0, sv.shape[0], 400)] + rng.normal(0.0, 0.5, (400, sv.shape[1]))
    d = R.decision_values(model, cand)[:, p]
    pos, neg = np.flatnonzero(d > 0), np.flatnonzero(d < 0)
    assert len(pos) and len(neg), "pair %d never changes sign" % p
    a, b = cand[pos[0]], cand[neg[0]]

    def g(t, k):
        x = (a + t * (b - a))[None, :]
        return float(R.decision_values(model, x)[0, p] - k * R.dec_bound(model, x)[0, p]), x[0]

    X = []
    for k in ks:
        lo, hi = 0.0, 1.0  # g(lo) > 0 >= g(hi)
        assert g(lo, k)[0] > 0 and g(hi, k)[0] <= 0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if g(mid, k)[0] > 0:
                lo = mid
            else:
                hi = mid
        X.append(min((g(lo, k), g(hi, k)), key=lambda r: abs(r[0]))[1])
    X = np.array(X)
    ratio = exact_dec(model, X)[1] / R.dec_bound(model, X)
    others = np.delete(np.abs(ratio), p, axis=1)
    assert others.size == 0 or others.min() >= OTHER_PAIRS, others.min()
    return X, ratio[:, p]
