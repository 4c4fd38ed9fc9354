"""Edge cases of Naive Bayes and Decision Tree on the device (csrc/gnb.hip: dsp_gnb_fit, dsp_gnb_predict;
csrc/tree.hip: dsp_tree_predict): the exact value of the joint log likelihood's contract, models at every
dimension and class count where the kernel or its staging takes another path, queries placed a chosen
multiple of the certificate's threshold from a tie, the numeric ends of (x - theta)^2 / var, node tables
on either side of the LDS-resident walk, a stump per float32 threshold edge, and the fit's tile, batch,
column and class-slot edges (a plain helper module like tests/svc_edge_cases.py: no test, no fixture; it
never touches the device library).  tests/test_nb_tree_edges_host.py pins on the CPU that every case hits
what it claims; tests/test_gpu_nb_tree_edges.py runs them.

A Naive Bayes model is a dict in tests/nb_tree_reference.py's form with a ``name`` (the key of the exact
values' cache); a tree is that module's dict.
"""
import decimal

import numpy as np

import nb_tree_reference as R

PREC = 60                 # decimal digits of exact_jll
EXACT_BUDGET = 400_000    # model elements (C x D x rows) a check spends on exact_jll ...
EXACT_MIN_ROWS = 3        # ... but never fewer rows than this
_CTX = decimal.Context(prec=PREC, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)
_MODEL_DEC = {}
_EXACT = {}


def constants(m):
    """(log_prior, nconst): the doubles the ABI receives (a zero prior gives -inf without a warning)."""
    with np.errstate(all="ignore"):
        return R.gnb_constants(m)


def _dec(v):
    return decimal.Decimal(float(v))


def exact_jll(m, X, classes=None):
    """The contract of include/dsp_audiorec.h, log_prior + (nconst - 1/2 sum_d (x_d - theta_cd)^2 / var_cd),
    in decimal arithmetic at 60 digits from the same log_prior and nconst doubles: Decimal(float) is exact,
    a difference and its square are exact or rounded at 1e-60, a quotient is rounded at 1e-60 -- no log is
    taken.  Returns (decimals [Nq][len(classes)], their nearest doubles); ``classes`` defaults to all.
    Rows, theta and var are finite (var > 0); log_prior may be -inf."""
    X = np.atleast_2d(np.asarray(X, np.float64))
    key = m["name"]
    if key not in _MODEL_DEC:
        lp, nc = constants(m)
        _MODEL_DEC[key] = ([[_dec(v) for v in r] for r in m["theta"]], [[_dec(v) for v in r] for r in m["var"]],
                           [_dec(v) for v in lp], [_dec(v) for v in nc])
    theta, var, lp, nc = _MODEL_DEC[key]
    cls = list(range(len(lp))) if classes is None else list(classes)
    ctx, zero, half = _CTX, decimal.Decimal(0), decimal.Decimal("0.5")
    out = []
    for row in X:
        rk, q, vals = row.tobytes(), None, []
        for c in cls:
            ck = (key, c, rk)
            if ck not in _EXACT:
                if q is None:
                    q = [_dec(v) for v in row]
                Q = zero
                for x, t, v in zip(q, theta[c], var[c]):
                    d = ctx.subtract(x, t)
                    Q = ctx.add(Q, ctx.divide(ctx.multiply(d, d), v))
                _EXACT[ck] = ctx.add(lp[c], ctx.subtract(nc[c], ctx.multiply(half, Q)))
            vals.append(_EXACT[ck])
        out.append(vals)
    return out, np.array([[float(v) for v in r] for r in out], np.float64).reshape(len(out), len(cls))


def exact_rows(m, Nq):
    """The rows a check spends exact_jll on: all of them while C x D x Nq stays inside EXACT_BUDGET, else
    EXACT_BUDGET's worth (at least EXACT_MIN_ROWS) spread from the first row to the last; the other rows
    are compared with scikit-learn's and the numpy restatement's values, within the same bound."""
    n = max(EXACT_MIN_ROWS, EXACT_BUDGET // max(m["theta"].size, 1))
    if n >= Nq:
        return np.arange(Nq)
    return np.unique(np.linspace(0, Nq - 1, n).round().astype(np.int64))


def margin_ratio(dec_row, bound_row):
    """(winner, ratio) of one row's exact scores: the first index of the largest, and the smallest over the
    other classes of (jll_w - jll_c) / (SAFETY (bound_w + bound_c)), the margin in units of the
    certificate's threshold (inf for C = 1).  The quotient alone is taken in fp64."""
    w = max(range(len(dec_row)), key=lambda c: (dec_row[c], -c))
    ratio = np.inf
    for c in range(len(dec_row)):
        if c != w:
            ratio = min(ratio, float(dec_row[w] - dec_row[c]) / (R.SAFETY * (bound_row[w] + bound_row[c])))
    return w, ratio


# ---- models ----------------------------------------------------------------------------------------
def hand_model(C, D, seed, name=None):
    """A model written directly: centres a few deviations apart, variances in [0.5, 2), uneven priors,
    labels 1, 4, 7, ..."""
    rng = np.random.default_rng(seed)
    prior = rng.uniform(0.5, 1.5, C)
    return dict(theta=rng.normal(0.0, 3.0 / np.sqrt(D), (C, D)), var=rng.uniform(0.5, 2.0, (C, D)),
                class_prior=prior / prior.sum(), classes=np.arange(C) * 3 + 1,
                name=name or "hand-%d-%d-%d" % (C, D, seed))


def variant(m, name, **changes):
    """A copy of ``m`` with some arrays replaced (its own name: its own exact values)."""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m.items()}
    out.update(changes)
    out["name"] = m["name"] + "/" + name
    return out


def as_sklearn(m):
    """A GaussianNB holding the model's arrays, as GaussianNB.fit leaves them."""
    from sklearn.naive_bayes import GaussianNB
    nb = GaussianNB()
    nb.theta_, nb.var_, nb.class_prior_ = m["theta"], m["var"], m["class_prior"]
    nb.classes_, nb.n_features_in_ = m["classes"], m["theta"].shape[1]
    nb.class_count_ = np.ones(len(m["classes"]))
    nb.epsilon_ = 0.0
    return nb


_FITTED = {}


def fitted(C, D, per_class=40):
    """(the scikit-learn GaussianNB, its arrays): C overlapping Gaussian classes, fitted once per shape."""
    key = (C, D, per_class)
    if key not in _FITTED:
        from sklearn.naive_bayes import GaussianNB
        rng = np.random.default_rng(700 + 31 * C + D)
        centres = rng.normal(0.0, 1.2, (C, D))
        X = np.concatenate([c + rng.normal(0.0, 1.0, (per_class + i, D)) for i, c in enumerate(centres)])
        y = np.repeat(np.arange(C) * 2 + 3, per_class + np.arange(C))
        nb = GaussianNB().fit(X, y)
        _FITTED[key] = (nb, dict(theta=nb.theta_, var=nb.var_, class_prior=nb.class_prior_, classes=nb.classes_,
                                 name="fitted-%d-%d-%d" % key))
    return _FITTED[key]


def queries(m, Nq, seed):
    """Nq rows a deviation or so from the centres: every class wins somewhere, most margins are large."""
    rng = np.random.default_rng(seed)
    C, D = m["theta"].shape
    return m["theta"][rng.integers(0, C, Nq)] + rng.normal(0.0, 1.0, (Nq, D))


# gnb_predict_kernel<16 | 32 | 0> at D <= 16, <= 32 and above; G = 2048 / D classes per LDS stage
# (2 | 1 at D = 1024 | 1025); a class in chunks of 2048 above D = 2048, a whole number of chunks at 4096
DIMS = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096)
DIM_C = 3
# class counts that end a stage exactly and one past it: G = 62 at D = 33, G = 2 at D = 1024
STAGE_CASES = ((61, 33), (62, 33), (63, 33), (64, 33), (2, 1024), (3, 1024))
CORNER = (64, 4096)
# GNB_T = 128 rows per workgroup: one short, full, one over (the second's idle lanes shadow its only row), 257
QUERY_COUNTS = (0, 1, 127, 128, 129, 257)
GNB_STAGE, GNB_T = 2048, 128


def kernel_form(C, D):
    """(DP, chunk, G, stages over the classes, chunks per class) as csrc/gnb.hip selects them."""
    DP = 16 if D <= 16 else 32 if D <= 32 else 0
    chunk = DP if DP else min(D, GNB_STAGE)
    G = GNB_STAGE // chunk
    return DP, chunk, G, -(-C // G), -(-D // chunk)


def shape_model(C, D):
    return hand_model(C, D, 1000 * C + D)


def shape_cases():
    return [(DIM_C, D) for D in DIMS] + list(STAGE_CASES) + [CORNER]


# ---- the certificate's threshold -------------------------------------------------------------------
BAND_UNDER = (0.1, -0.25, 0.4, -0.44)      # |exact margin| / threshold: at most 0.5 with the targets' tolerance
BAND_OVER = (2.1, -3.0, 30.0, -1000.0)     # at least 2
MUST_NOT = 0.5   # the device's jll is within one bound of exact on each side, so its margin is at most
                 # 0.5 x 4 (b_w + b_c) + (b_w + b_c) = 3 (b_w + b_c) < SAFETY (b_w + b_c): must not be certified
MUST = 2.0       # its margin is at least 2 x 4 (b_w + b_c) - (b_w + b_c) = 7 (b_w + b_c): its own bounds
                 # (from its own Q, within rounding of the restatement's) are passed with room -- must be
OTHERS = 8.0     # every class outside the pair trails both of the pair by at least this many thresholds


def _pair_margin(m, x, a, b):
    d = exact_jll(m, x[None, :], (a, b))[0][0]
    bound = R.gnb_bound(m, x[None, :])[0]
    return d[0] - d[1], R.SAFETY * (bound[a] + bound[b])


def banded_queries(m, pair):
    """(X [10, D], ratio [10]): rows that differ in one coordinate, bisected so that the exact
    jll_a - jll_b stands at BAND_UNDER + BAND_OVER times the certificate's threshold
    SAFETY (bound_a + bound_b) (positive: a leads), then the two adjacent doubles either side of the tie
    itself.  ratio is the exact margin over the threshold at each row.  Every other class trails by
    OTHERS thresholds or more (asserted), so the pair alone decides the certificate."""
    a, b = pair
    base = 0.5 * (m["theta"][a] + m["theta"][b])
    j = int(np.argmax(np.abs(m["theta"][a] - m["theta"][b]) / np.sqrt(m["var"][a] + m["var"][b])))
    lo_x, hi_x = sorted((m["theta"][a][j], m["theta"][b][j]))
    grid = np.linspace(lo_x - 1.0, hi_x + 1.0, 401)
    rows = np.tile(base, (len(grid), 1))
    rows[:, j] = grid
    jll = R.gnb_jll(m, rows)
    s = np.sign(jll[:, a] - jll[:, b])
    top2 = np.sort(np.argsort(jll, axis=1)[:, -2:], axis=1)
    ok = np.flatnonzero((s[:-1] * s[1:] < 0) & np.all(top2[:-1] == sorted(pair), axis=1))
    assert len(ok), "classes %d and %d never lead together along coordinate %d" % (a, b, j)
    i = int(ok[0])
    sign = float(s[i])  # the margin falls (sign > 0) or rises along the coordinate

    def g(x, k):
        row = base.copy()
        row[j] = x
        margin, thr = _pair_margin(m, row, a, b)
        return sign * float(margin - decimal.Decimal(k * thr)), row

    X = []
    for k in BAND_UNDER + BAND_OVER + (0.0,):
        lo, hi = float(grid[i]), float(grid[i + 1])  # g(lo) > 0 >= g(hi)
        assert g(lo, k)[0] > 0 and g(hi, k)[0] <= 0
        while True:
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if g(mid, k)[0] > 0:
                lo = mid
            else:
                hi = mid
        if k == 0.0:
            X += [g(lo, k)[1], g(hi, k)[1]]
        else:
            X.append(min((g(lo, k), g(hi, k)), key=lambda r: abs(r[0]))[1])
    X = np.array(X)
    dec = exact_jll(m, X)[0]
    bound = R.gnb_bound(m, X)
    ratio = np.array([float(d[a] - d[b]) / (R.SAFETY * (bd[a] + bd[b])) for d, bd in zip(dec, bound)])
    for d, bd in zip(dec, bound):
        for c in range(len(d)):
            if c not in pair:
                assert float(min(d[a], d[b]) - d[c]) >= OTHERS * R.SAFETY * (max(bd[a], bd[b]) + bd[c]), (pair, c)
    return X, ratio


def band_cases():
    """(name, C, D, pair): C = 2, each pair of C = 3, one pair of C = 10 with the rows read from memory."""
    return [("c2", 2, 4, (0, 1)), ("c3-01", 3, 4, (0, 1)), ("c3-02", 3, 4, (0, 2)), ("c3-12", 3, 4, (1, 2)),
            ("c10-d40", 10, 40, (3, 7))]


def mirror_model():
    """Two classes alike but for theta[:, 2] = +-1.5: a row with x_2 = 0 is an exact tie in exact
    arithmetic and in fp64 ((0 - 1.5)^2 = (0 + 1.5)^2), so the scores' bits are equal."""
    m = hand_model(2, 5, 77, name="mirror")
    m["theta"][1], m["var"][1] = m["theta"][0], m["var"][0]
    m["theta"][0, 2], m["theta"][1, 2] = 1.5, -1.5
    m["class_prior"] = np.array([0.5, 0.5])
    return m


# ---- numeric ends ----------------------------------------------------------------------------------
NONFINITE = (np.nan, np.inf, -np.inf)
HUGE = 1.7e308  # finite, but (x - theta)^2 is not


def numeric_cases():
    """name -> (model, X, certified [Nq] (1, 0), pred [Nq] (a class index, or -1: not stated)).  The
    outcomes are written from the contract: a row is certified iff every score is finite and the winner
    leads every class by more than the threshold; pred is the first index of the largest score.
      base rows   B[0..5]: queries(base) -- a clear winner among the classes 0..2 of an ordinary model
      on1         class 1's own centre"""
    base = hand_model(3, 5, 11, name="numeric")
    B = queries(base, 6, 12)
    win = np.argmax(exact_jll(base, B)[1], axis=1)
    on1 = base["theta"][1].copy()
    out = {}

    def put(name, m, X, cert, pred):
        out[name] = (m, np.array(X, np.float64), np.array(cert, np.int32), np.array(pred, np.int64))

    # var = 1e-300 for class 1: nconst_1 = +1722, Q_1 ~ 1e300 d^2.  An ordinary row has Q_1 finite, jll_1
    # about -1e300: certified, class 1 last.  Class 1's centre has Q_1 = 0 and wins by 1700.  A row 1e5
    # from it has d^2 / var = 1e310 = inf, jll_1 = -inf: uncertified
    tiny = variant(base, "var=1e-300", var=np.where(np.arange(3)[:, None] == 1, 1e-300, base["var"]))
    far = B[0].copy()
    far[0] = 1e5
    put("var_1e-300", tiny, [B[0], B[1], on1, far], [1, 1, 1, 0], [-1, -1, 1, -1])
    # var = 1e300 for class 1: Q_1 ~ 0, nconst_1 = -1732, jll_1 ~ -1733 for every row.  Ordinary rows:
    # certified, class 1 last.  A row 1e20 out has Q = 1e40 for the others: class 1 wins, certified
    flat = variant(base, "var=1e300", var=np.where(np.arange(3)[:, None] == 1, 1e300, base["var"]))
    out20 = B[0].copy()
    out20[4] = 1e20
    put("var_1e300", flat, [B[0], B[1], out20], [1, 1, 1], [-1, -1, 1])
    # subnormal var for class 1: d^2 / 1e-310 overflows for every d^2 > 1.8e-2 (jll_1 = -inf: uncertified),
    # and is 0 / 1e-310 = 0 at the class's own centre: nconst_1 = +1780 wins, certified
    sub = variant(base, "var=1e-310", var=np.where(np.arange(3)[:, None] == 1, 1e-310, base["var"]))
    put("var_subnormal", sub, [B[0], B[1], on1], [0, 0, 1], [-1, -1, 1])
    # theta = +-1e150 in one column of class 1: d^2 = 1e300 is finite, jll_1 ~ -5e299: certified, class 1 last;
    # +-1e300: d^2 overflows, jll_1 = -inf: no row is certified
    for col, val in ((0, 1e150), (4, -1e150), (0, 1e300), (4, -1e300)):
        th = base["theta"].copy()
        th[1, col] = val
        ok = int(abs(val) < 1e154)
        put("theta_%g" % val, variant(base, "theta=%g" % val, theta=th), B, [ok] * 6, list(win) if ok else [-1] * 6)
    # a query far enough out that only some classes reach -inf: class 0 has var 1e-4 in column 0, so at
    # x_0 = 1e153 (d^2 = 1e306) Q_0 = inf while Q_1 and Q_2 stay finite.  A score is -inf: uncertified
    va = base["var"].copy()
    va[0, 0] = 1e-4
    partial = B[:2].copy()
    partial[:, 0] = (1e153, -1e153)
    put("partial_inf", variant(base, "var00=1e-4", var=va), partial, [0, 0], [-1, -1])
    # two identical classes (0 and 2) and rows at their centre: equal bits, the first index, margin 0
    dup = variant(base, "dup", theta=base["theta"][[0, 1, 0]], var=base["var"][[0, 1, 0]],
                  class_prior=np.array([0.3, 0.4, 0.3]))
    near0 = base["theta"][0] + np.array([[0.0] * 5, [0.1, 0, 0, 0, -0.1], [0, 0.2, 0, 0, 0]])
    put("duplicate_classes", dup, near0, [0, 0, 0], [0, 0, 0])
    both = variant(base, "dup2", theta=base["theta"][[1, 1]], var=base["var"][[1, 1]], class_prior=np.array([0.5, 0.5]),
                   classes=base["classes"][:2])
    put("two_equal_classes", both, B, [0] * 6, [0] * 6)
    # the mirror model's exact ties (x_2 = 0), and rows well off the mirror plane
    mm = mirror_model()
    T = queries(mm, 4, 13)
    T[:2, 2] = 0.0
    T[2, 2], T[3, 2] = 1.0, -1.0
    put("exact_tie", mm, T, [0, 0, 1, 1], [0, 0, 0, 1])
    # a class whose theta and var are NaN (dsp_gnb_fit's empty class), first and middle: its score is NaN
    for c in (0, 1):
        nan = variant(base, "nan%d" % c, theta=np.where(np.arange(3)[:, None] == c, np.nan, base["theta"]),
                      var=np.where(np.arange(3)[:, None] == c, np.nan, base["var"]))
        put("nan_class_%d" % c, nan, B, [0] * 6, [-1] * 6)
    # log_prior = -inf (a zero prior), first and last: that score is -inf, so no row is certified; the label
    # is still the first index of the largest score
    for c in (0, 2):
        pr = base["class_prior"].copy()
        pr[c] = 0.0
        zero = variant(base, "prior%d=0" % c, class_prior=pr / pr.sum())
        with np.errstate(all="ignore"):
            want = np.argmax(R.gnb_jll(zero, B), axis=1)
        assert np.all(want != c)
        put("zero_prior_%d" % c, zero, B, [0] * 6, list(want))
    # C = 1: certified whenever the score is finite
    one = variant(base, "c1", theta=base["theta"][:1], var=base["var"][:1], class_prior=np.array([1.0]),
                  classes=base["classes"][:1])
    big = B[2].copy()
    big[1] = 1e200
    put("one_class", one, [B[0], B[1], big], [1, 1, 0], [0, 0, 0])
    return out


def nonfinite_cells(D):
    """(row, column) of Nq = 129 rows: the first column, the last, and -- where there is one -- a column
    past 32; row 128 is alone in its workgroup, the row its idle lanes shadow."""
    return [(3, 0), (70, D - 1), (128, D - 1)] + ([(100, 33), (127, 0)] if D > 33 else [(127, 0)])


# ---- trees -----------------------------------------------------------------------------------------
TREE_T, TREE_LDS_NODES = 256, 4096
TREE_QUERY_COUNTS = (0, 1, 255, 256, 257)
CHAIN_D = 2


def chain_tree(n_nodes, extra=0):
    """A right-leaning chain: node 2j tests feature j % 2 against j + 0.5, its left child 2j + 1 is a leaf,
    its right child 2j + 2 the next test; the last node is a leaf at depth (n_nodes - 1) / 2.  ``extra``
    unreachable leaves are appended.  max_depth is the depth."""
    assert n_nodes % 2 == 1
    k = (n_nodes - 1) // 2
    n = n_nodes + extra
    left, right = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    feature, thr = np.full(n, -2, np.int32), np.full(n, -2.0)
    j = np.arange(k)
    left[2 * j], right[2 * j], feature[2 * j], thr[2 * j] = 2 * j + 1, 2 * j + 2, j % CHAIN_D, j + 0.5
    return dict(left=left, right=right, feature=feature, threshold=thr,
                leaf_class=(np.arange(n) % 7).astype(np.int32), max_depth=k, classes=np.arange(7))


def chain_queries(depth, Nq, seed=5):
    """Rows [d, d]: the walk goes right at tests 0 .. d - 1 and left at test d, ending at leaf 2 d + 1 at depth
    d + 1 (d >= depth: at the last leaf, depth ``depth``).  The first rows stand at 0, depth - 2 .. depth + 1;
    the others are spread over the chain."""
    rng = np.random.default_rng(seed)
    d = np.concatenate([[0, depth - 2, depth - 1, depth, depth + 1], rng.integers(0, depth + 2, Nq)])[:Nq]
    return np.repeat(d.astype(np.float64)[:, None], CHAIN_D, axis=1)


def chain_leaf(depth, X, max_depth):
    """What the contract says of a chain_queries row on chain_tree of that depth: leaf 2 d + 1 after d + 2
    nodes, the last leaf 2 depth after depth + 1 nodes; -1 when that is more than max_depth + 1 nodes."""
    d = X[:, 0].astype(np.int64)
    leaf = np.where(d < depth, 2 * d + 1, 2 * depth)
    visited = np.where(d < depth, d + 2, depth + 1)
    return np.where(visited <= max_depth + 1, leaf, -1)


F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)
SUB_MIN = float(np.finfo(F32).smallest_subnormal)  # 2^-149
MIDPOINT = FLT_MAX + 2.0 ** 103                   # halfway from FLT_MAX to 2^128: rounds to even, which is inf
THRESHOLDS = (0.0, -0.0, SUB_MIN, 0.5 * SUB_MIN, 1e-40, 1.5e-40, 1e-50, -1e-50, FLT_MAX,
              float(np.nextafter(FLT_MAX, np.inf)), float(np.nextafter(FLT_MAX, 0.0)), 1e40, -1e40, np.inf, -np.inf,
              np.nan)


def stump(threshold, D=1, feature=0):
    """Root, left leaf 1 (class 0), right leaf 2 (class 1)."""
    return dict(left=np.array([1, -1, -1], np.int32), right=np.array([2, -1, -1], np.int32),
                feature=np.array([feature, -2, -2], np.int32), threshold=np.array([threshold, -2.0, -2.0]),
                leaf_class=np.array([-9, 0, 1], np.int32), max_depth=1, classes=np.array([0, 1]), D=D)


def stump_values(t):
    """The doubles a stump with threshold t is asked about: t, the float32 f nearest it with its float32
    neighbours, the doubles next to f (they round onto it from each side), +-1e-46 (they round to +-0),
    the midpoint between FLT_MAX and 2^128 with its two neighbours, and some ordinary values."""
    with np.errstate(all="ignore"):
        f = F32(np.clip(t, -FLT_MAX, FLT_MAX)) if np.isfinite(t) else F32(0.0 if np.isnan(t) else np.sign(t) * FLT_MAX)
        f32 = [f, np.nextafter(f, F32(np.inf)), np.nextafter(f, F32(-np.inf))]
        v = [t] + [float(x) for x in f32]
        v += [float(np.nextafter(np.float64(f), np.inf)), float(np.nextafter(np.float64(f), -np.inf))]
    v += [1e-46, -1e-46, 0.0, -0.0, SUB_MIN, -SUB_MIN, 1.0, -1.0, FLT_MAX, -FLT_MAX]
    v += [MIDPOINT, float(np.nextafter(MIDPOINT, 0.0)), float(np.nextafter(MIDPOINT, np.inf)), -MIDPOINT]
    return np.array([x for x in v if not np.isnan(x)], np.float64)


def stump_leaf(t, values):
    """The contract, one row at a time: v = (double)(float)x; -1 unless v is finite; leaf 1 iff v <= t (a
    NaN threshold compares false: leaf 2)."""
    out = []
    for x in values:
        with np.errstate(over="ignore"):
            v = float(F32(x))
        out.append(-1 if not np.isfinite(v) else 1 if v <= t else 2)
    return np.array(out, np.int64)


_SUBNORMAL = {}


def subnormal_tree(seed):
    """(DecisionTreeClassifier, queries): fitted on three columns of float32-subnormal values k x 1e-40
    (k = 1 .. 8, one column negative), so its thresholds lie between float32 subnormals; queried at the
    values, a float32 ulp either side, and -- in the tested column of some rows -- each threshold, the
    doubles next to it, the float32 nearest it and that one's float32 neighbours."""
    if seed not in _SUBNORMAL:
        from sklearn.tree import DecisionTreeClassifier
        rng = np.random.default_rng(seed)
        K = rng.integers(1, 9, (240, 3)).astype(np.float64)
        K[:, 2] = -K[:, 2]
        X = K * 1e-40
        y = ((K[:, 0] > 4) ^ (K[:, 1] <= 2)).astype(np.int64) + 2 * (K[:, 2] < -6)
        tree = DecisionTreeClassifier(random_state=42).fit(X, y)
        inner = np.flatnonzero(tree.tree_.children_left != -1)
        Q = [X[:60]]
        for step in (F32(np.inf), F32(-np.inf)):
            Q.append(np.nextafter(X[:40].astype(F32), step).astype(np.float64))
        for f, t in zip(tree.tree_.feature[inner], tree.tree_.threshold[inner]):
            rows = X[rng.integers(0, len(X), 6)].copy()
            t32 = F32(t)
            rows[:, f] = (t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf), float(t32),
                          float(np.nextafter(t32, F32(np.inf))), float(np.nextafter(t32, F32(-np.inf))))
            Q.append(rows)
        _SUBNORMAL[seed] = (tree, np.concatenate(Q))
    return _SUBNORMAL[seed]


# ---- fit -------------------------------------------------------------------------------------------
# gnb_fit_kernel: tiles of 128 rows, batches of 8 rows, 16 columns and 8 class slots (one of them "all
# rows": a workgroup's worth is C = 7, the second begins at C = 8) per workgroup
FIT_N = (1, 2, 7, 8, 9, 127, 128, 129, 255, 256, 257)
FIT_D = (2, 15, 16, 17, 32, 33)
FIT_C = (1, 7, 8, 9, 15, 16, 63, 64)
FIT_WIDE = (9, 4096, 3)  # N, D, C


def fit_labels(rng, N, C):
    """Every class present while N >= C (else the first N), interleaved."""
    y = np.concatenate([np.arange(min(N, C)), rng.integers(0, C, max(N - C, 0))])
    rng.shuffle(y)
    return y.astype(np.int32)


def fit_data(N, D, C, seed=None):
    rng = np.random.default_rng(10000 * N + 100 * D + C if seed is None else seed)
    X = rng.normal(0.0, 1.0, (N, D)) * rng.uniform(0.1, 10.0, D) + rng.normal(0.0, 3.0, D)
    return X, fit_labels(rng, N, C)


def fit_shape_cases():
    """(N, D, C): each N at C = 3 and D = 17 (two column groups), each D at N = 129, each C at N = 257 (C = 1:
    N = 40), and the widest row."""
    out = [(N, 17, min(3, N)) for N in FIT_N] + [(129, D, 3) for D in FIT_D]
    out += [(40 if C == 1 else 257, 15, C) for C in FIT_C] + [FIT_WIDE]
    return out


def fit_value_cases():
    """name -> (X, y, C, scikit-learn accepts it).  257 rows (three tiles), 17 columns, 9 classes (two slot
    groups) unless said."""
    out = {}
    X, y = fit_data(257, 17, 9, seed=1)
    for name, gone in (("empty_first", 0), ("empty_middle", 4), ("empty_last", 8)):
        yy = y.copy()
        yy[yy == gone] = (gone + 1) % 9
        out[name] = (X, yy, 9, False)
    Z = X.copy()
    Z[:, 3] = -0.0
    Z[:, 16] = -0.0
    out["minus_zero_column"] = (Z, y, 9, True)
    K = X.copy()
    K[:, 5] = y * 0.5 + 1.0  # constant within each class: variance exactly 0 there
    out["constant_within_class"] = (K, y, 9, True)
    H = X.copy()
    H[:, 2] = H[:, 2] * 1e200  # squares overflow: var and epsilon are inf
    H[:, 16] = 1e200           # a constant 1e200: deviations are 0
    out["squares_overflow"] = (H, y, 9, True)
    P = X.copy()
    P[100, 7], P[200, 7] = np.nan, np.inf
    out["nan_and_inf"] = (P, y, 9, False)
    return out


def same_values(a, b):
    """Equal bits, or both NaN (a NaN's sign and payload are the host's or the device's own)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
