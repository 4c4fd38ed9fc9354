"""CPU tests of the scaled forward-backward definition (tests/dhmm_fb_reference.py) and of the host side on
it: the two forms of the restatement agree bit for bit, the dyadic corpus equals a fractions.Fraction brute
force over all state paths exactly, the negative log agrees with a log-domain forward pass, the deep
underflow set, the label rule, DhmmProbSet's build on hand-worked cases, to_costs, dhmm_nll, the loaded
library's argument checks and the classifier's new constructor arguments."""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest

import dhmm_fb_reference as R
import dhmm_reference as D
from device_outputs import csr

ULP = 2.0 ** -52


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def same(got, want, names):
    for g, w, name in zip(got, want, names):
        g, w = (bits(v) if np.asarray(v).dtype == np.float64 else np.asarray(v) for v in (g, w))
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


STATES = np.array([3, 1, 5, 2, 4, 0, 6, 3], np.int32)  # n_states 0 and Smax + 1 among them


@functools.lru_cache(maxsize=None)
def random_corpus():
    """Eight models (Smax = 5) over K = 6 symbols with a tenth of their entries zero; 120 rows of up to 12
    frames, lengths from 1 on (so around every S), four rows with a symbol outside the alphabet, two with a
    bad length."""
    model = R.random_probs(STATES, 5, 6, seed=11, zeros=0.10)
    sym, n = D.random_symbols(120, 12, 6, seed=12)
    sym[3, 0], sym[4, n[4] - 1], sym[5, n[5] // 2], sym[6, 0] = 6, -1, 2 ** 31 - 1, -2 ** 31
    n[[7, 8]] = [0, 13]
    return model, sym, n


def test_the_two_forms_agree():
    model, sym, n = random_corpus()
    rows = R.forward(model, sym, n, form="rows")
    same(R.forward(model, sym, n, form="loop"), rows, ("mant", "expo", "label"))
    mant, expo, label = rows
    assert (mant[[3, 4, 5, 6, 7, 8]] == 0).all() and (label[[3, 4, 5, 6, 7, 8]] == -1).all()
    assert (mant[:, [5, 6]] == 0).all() and ((mant == 0) | ((mant >= 0.5) & (mant < 1))).all() and (expo[mant == 0] == 0).all()
    # conditions on the corpus, from the reference alone: of the pairs with n >= S at least 5 % have zero
    # likelihood and at least 50 % have not
    ok = np.ones(len(n), bool)
    ok[[3, 4, 5, 6, 7, 8]] = False
    S = STATES[None, :]
    long_enough = ok[:, None] & (n[:, None] >= S) & (S >= 1) & (S <= 5)
    zero = (mant == 0) & long_enough
    assert zero.sum() >= 0.05 * long_enough.sum() and (long_enough & ~zero).sum() >= 0.5 * long_enough.sum()
    assert (mant[ok[:, None] & (n[:, None] < S)] == 0).all()


def test_the_two_forms_agree_on_the_expected_counts():
    model, sym, n = random_corpus()
    rng = np.random.default_rng(13)
    groups = [rng.integers(0, len(n), k).tolist() for k in (30, 1, 40, 25, 0, 9, 12, 20)]
    groups[2] += [-1, len(n), 3, 4, 5, 6, 7, 8]
    start, members = csr(groups)
    names = ("mant", "expo", "gamma", "occ_emit", "n_valid", "valid")
    rows = R.expect(model, sym, n, start, members, form="rows")
    same(R.expect(model, sym, n, start, members, form="loop"), rows, names)
    mant, expo, gamma, occ, n_valid, valid = rows
    assert 40 < valid.sum() < len(members) and n_valid.sum() == valid.sum() and n_valid[[5, 6]].tolist() == [0, 0]
    assert not valid[start[3] - 8:start[3]].any() and not np.isnan(gamma).any() and not occ[[5, 6]].any()
    # every valid frame's posteriors add up to one, and the occupancy to the frames of the valid members
    owner = np.repeat(np.arange(8), np.diff(start))
    for p in np.flatnonzero(valid):
        k = n[members[p]]
        assert np.abs(gamma[p, :k].sum(axis=1) - 1).max() < 8 * ULP and not gamma[p, k:].any()
        assert not gamma[p, :, STATES[owner[p]]:].any()
        # the forced start and end: g * (1 / g), one division and one product away from 1
        assert abs(gamma[p, 0, 0] - 1) <= 2 * ULP and abs(gamma[p, k - 1, STATES[owner[p]] - 1] - 1) <= 2 * ULP
    assert not gamma[~valid].any()
    for c in range(8):
        frames = n[members[start[c]:start[c + 1]][valid[start[c]:start[c + 1]]]].sum()
        assert abs(occ[c].sum() - frames) <= 1e-12 * max(frames, 1)
    # the list order is part of the definition: a permuted list changes occ_emit's bits
    perm = np.r_[start[1] - 1:-1:-1, start[1]:len(members)]
    other = R.expect(model, sym, n, start, members[perm])
    assert not np.array_equal(bits(other[3][0]), bits(occ[0])) and np.allclose(other[3], occ, rtol=1e-12, atol=0)


def dyadic_cases():
    """400 (model, row) cases with all probabilities multiples of 1/8, n <= 8 and S <= 4."""
    rng = np.random.default_rng(21)
    for i in range(400):
        S, K = int(rng.integers(1, 5)), int(rng.integers(1, 4))
        model = R.dyadic_probs([S], S, K, seed=1000 + i)
        n = int(rng.integers(1, 9))
        yield model, rng.integers(0, K, n).astype(np.int32)


def test_dyadic_exactness():
    """(mant, expo) equals the brute force over all state paths EXACTLY: every product and sum there has at
    most 45 significant bits, and rescaling by a power of two is exact.  gamma lies within 4 ulp of 1.0
    (absolute) of the exact posterior: two multiplies, one sum of <= 4 terms and one division stand between."""
    zero = nonzero = 0
    worst = 0.0
    for model, row in dyadic_cases():
        B, a, d = model.one(0)
        total, post = R.brute_force(row, B, a, d)
        for form in ("loop", "rows"):
            mant, expo, gamma, _, _, valid = R.expect(model, row[None, :], [len(row)], [0, 1], [0], form=form)
            assert Fraction(float(mant[0])) * Fraction(2) ** int(expo[0]) == total, (row, form)
            assert bool(valid[0]) == (total != 0)
            if total != 0:
                err = max(abs(Fraction(float(gamma[0, t, s])) - post[t][s]) for t in range(len(row)) for s in range(len(a)))
                worst = max(worst, float(err))
        zero, nonzero = zero + (total == 0), nonzero + (total != 0)
    assert zero >= 40 and nonzero >= 100
    print("worst posterior error %.3g" % worst)
    assert worst <= 4 * ULP


def test_nll_against_the_log_domain():
    """The scaled pass rounds three times per cell (two products and a sum feed the third product), so over
    n <= 1024 rows the likelihood's relative error is at most about 3 * 1024 * 2^-53 = 3.4e-13, which is also
    its nll's absolute error.  The log-domain side (np.logaddexp) accumulates about n * S * eps * |nll|: with
    n = 1024, S = 5 that is 1.1e-12 * |nll|.  The bound 1e-9 * max(1, |nll|) covers both about a thousand
    times over."""
    model = R.random_probs([5, 3, 1], 5, 7, seed=31, zeros=0.03)
    sym, n = D.random_symbols(12, 1024, 7, seed=32, lengths=[1024, 1000, 700, 300, 100, 40, 9, 5, 4, 3, 2, 1])
    mant, expo, _ = R.forward(model, sym, n)
    got = R.nll(mant, expo)
    finite = 0
    for i in range(len(n)):
        for c in range(3):
            with np.errstate(divide="ignore", invalid="ignore"):
                want = R.log_forward(sym[i, :n[i]], *model.one(c)) if n[i] >= model.n_states[c] else np.inf
            if np.isinf(want):
                assert np.isinf(got[i, c]), (i, c)
                continue
            finite += 1
            assert abs(got[i, c] - want) <= 1e-9 * max(1.0, abs(want)), (i, c, got[i, c], want)
    assert finite >= 12 and got[0].min() > 1000  # far below the smallest double as a plain probability


def test_deep_underflow():
    """Entries of 2^-300: the path to the last state falls more than 2^-1022 below the row maximum."""
    model, sym, n = R.underflow_set()
    rows = R.forward(model, sym, n, form="rows")
    same(R.forward(model, sym, n, form="loop"), rows, ("mant", "expo", "label"))
    mant, expo, label = rows
    # row 0 ends on the deep cell: a subnormal, non-zero result under models 0 and 2; zero under model 1
    # although the path 0 -> 1 -> 2 exists
    B, a, d = model.one(0)
    A = R.forward_loop(sym[0, :3], B, a, d)[2]
    assert 0 < A[2, 2] < 2.0 ** -1022 and mant[0, 0] >= 0.5 and expo[0, 0] < -1022
    A2 = R.forward_loop(sym[0, :3], *model.one(2))[2]
    exact = R.brute_force(sym[0, :3], *model.one(2))[0]
    got = Fraction(float(mant[0, 2])) * Fraction(2) ** int(expo[0, 2])
    assert 0 < A2[2, 2] < 2.0 ** -1022 and got != exact and abs(got / exact - 1) < 2.0 ** -20  # rounded into the subnormal grid
    assert R.brute_force(sym[0, :3], *model.one(1))[0] > 0 and mant[0, 1] == 0 and expo[0, 1] == 0
    # row 0: models 0 and 2 tie at 2^-1050 exactly (padv's 2^-40 is rounded away), the smaller index wins;
    # row 1: model 0's 0.5 * 2^-451 is the largest; row 2: 0.5 * 2^-1052 against 0.84 * 2^-1054
    assert label.tolist() == [0, 0, 0]
    # rows 1 and 2 pass the cell and end on a normal one
    assert (mant[1] >= 0.5).all() and mant[2, 0] >= 0.5 and mant[2, 1] == 0
    start, members = csr([[0, 1, 2], [0, 1, 2], [0, 1, 2]])
    names = ("mant", "expo", "gamma", "occ_emit", "n_valid", "valid")
    got = R.expect(model, sym, n, start, members, form="rows")
    same(R.expect(model, sym, n, start, members, form="loop"), got, names)
    # rows 0 and 2 under models 0 and 2: a non-zero likelihood, but D_{n-1} is the subnormal cell and 1 / D
    # overflows, so the member is not valid; no +inf and no NaN reaches any output
    assert got[5].tolist() == [False, True, False, False, True, False, False, True, False] and (got[0][[0, 2, 6, 8]] > 0).all()
    assert np.isfinite(got[2]).all() and np.isfinite(got[3]).all() and got[4].tolist() == [1, 1, 1]


def test_label_rule():
    """Two identical models: the smaller index; all-zero row: -1; the larger expo beats the larger mant."""
    model = R.random_probs([3, 3, 3], 3, 4, seed=41)
    model.pemit[1], model.pstay[1], model.padv[1] = model.pemit[0], model.pstay[0], model.padv[0]
    sym, n = D.random_symbols(20, 9, 4, seed=42, lo=3)
    n[:2] = [2, 1]
    mant, expo, label = R.forward(model, sym, n)
    assert (label[:2] == -1).all() and (mant[:2] == 0).all() and (label[2:] != 1).all() and (label[2:] == 2).any() and (label[2:] == 0).any()
    same((mant[:, 1], expo[:, 1]), (mant[:, 0], expo[:, 0]), ("mant", "expo"))
    assert R.label_of(np.array([[0.9, 0.5, 0.5, 0.0]]), np.array([[-3, -2, -2, 5]])).tolist() == [1]
    assert R.label_of(np.array([[0.5, 0.75, 0.75]]), np.array([[4, 4, 4]])).tolist() == [1]
    assert R.label_of(np.zeros((1, 3)), np.zeros((1, 3), np.int32)).tolist() == [-1]


def test_prob_set_build():
    from src.pipeline import DhmmProbSet
    occ = np.zeros((3, 2, 4))
    occ[0, 0] = [0.1, 0.2, 0.3, 1e-17]  # (0.1 + 0.2) + 0.3 + 1e-17 sequentially: 0.6000000000000001
    occ[0, 1] = [3.0, 0.0, 1.0, 0.0]
    occ[1, 0] = [2.0, 2.0, 0.0, 0.0]  # model 1 never saw its second state
    nv = np.array([1, 4, 0])
    p = DhmmProbSet(occ, nv, [2, 2, 1])
    seq = ((np.float64(0.1) + np.float64(0.2)) + np.float64(0.3)) + np.float64(1e-17)
    assert seq == 0.6000000000000001
    assert bits(p.pemit[0, 0, 0]) == bits((np.float64(0.1) + 0.5) / (seq + np.float64(0.5) * 4.0))
    # occ < n_valid (0.6 against 1, as rounding can leave it): the clamp, not a negative probability
    assert p.pstay[0, 0] == 1e-3 and p.padv[0, 0] == 1.0 - 1e-3
    assert p.pstay[0, 1] == 0.75 and p.padv[0, 1] == 0.25
    assert p.pstay[1, 0] == 1e-3  # (4 - 4) / 4 = 0 -> the floor
    assert (p.pemit[1, 1] == 0.25).all() and p.pstay[1, 1] == 0.5  # an unseen state is uniform
    assert (p.pemit[2, 0] == 0.25).all() and p.pstay[2, 0] == 0.5 and not p.pemit[2, 1].any() and p.pstay[2, 1] == 0
    prev = DhmmProbSet.from_arrays(np.full((3, 2, 4), 0.25), np.full((3, 2), 0.7), np.full((3, 2), 0.3), [2, 2, 1])
    q = DhmmProbSet(occ, nv, [2, 2, 1], prev=prev)
    assert q.pstay[2, 0] == 0.7 and bits(q.padv[2, 0]) == bits(1.0 - np.float64(0.7)) and q.pstay[1, 1] == 0.5
    same((q.pemit, q.pstay[:2], q.padv[:2]), (p.pemit, p.pstay[:2], p.padv[:2]), ("pemit", "pstay", "padv"))
    # 64 symbols: numpy's pairwise np.sum has other bits than the sequential sum the definition asks for
    row = np.random.default_rng(54).uniform(0, 1, 64)
    seq = np.add.accumulate(row)[-1]
    assert seq != np.sum(row)
    wide = DhmmProbSet(row[None, None, :], [1], [1])
    assert bits(wide.pemit[0, 0, 0]) == bits((row[0] + np.float64(0.5)) / (seq + np.float64(0.5) * np.float64(64)))
    assert bits(wide.pstay[0, 0]) == bits((seq - 1.0) / seq)
    # the restatement, entry by entry, on real-valued and on integer counts
    rng = np.random.default_rng(51)
    occ, nv, S = rng.uniform(0, 30, (4, 5, 7)) * (rng.random((4, 5, 7)) < 0.7), np.array([9, 0, 3, 30]), [5, 2, 4, 1]
    for prev in (None, R.random_probs(S, 5, 7, seed=52)):
        pp = prev and DhmmProbSet.from_arrays(np.where(np.isnan(prev.pemit), 0, prev.pemit), prev.pstay, prev.padv, S)
        want = R.build_prob(occ, nv, S, 0.25, 0.01, prev)
        got = DhmmProbSet(occ, nv, S, alpha=0.25, trans_floor=0.01, prev=pp)
        valid = np.arange(5)[None, :] < np.array(S)[:, None]
        same((got.pemit, got.pstay, got.padv), (want.pemit, np.where(valid, want.pstay, 0), np.where(valid, want.padv, 0)),
             ("pemit", "pstay", "padv"))
    cnt = rng.integers(0, 9, (4, 5, 7))
    # built round by round beside a DhmmModelSet from the same integer counts, prev= included, it holds the same
    # models: a model without a valid member (n_valid 0) keeps the previous round's transitions in both
    from src.pipeline import DhmmModelSet
    first = rng.integers(1, 9, (4, 5, 7))
    p0, m0 = DhmmProbSet(first, [3, 2, 3, 4], S), DhmmModelSet(first, first.sum(axis=2), [3, 2, 3, 4], S)
    p1, m1 = DhmmProbSet(cnt, nv, S, prev=p0), DhmmModelSet(cnt, cnt.sum(axis=2), nv, S, prev=m0)
    assert nv[1] == 0 and p1.pstay[1, 0] == p0.pstay[1, 0] != 0.5
    c1 = p1.to_costs()
    same((c1.emit, c1.stay, c1.adv), (m1.emit, m1.stay, m1.adv), ("emit", "stay", "adv"))
    same((DhmmProbSet(cnt, nv, S).pemit,), (R.build_prob(cnt.astype(np.float64), nv, S).pemit,), ("pemit",))
    for bad in (dict(alpha=0.0), dict(trans_floor=0.5)):
        with pytest.raises(ValueError):
            DhmmProbSet(occ, nv, S, **bad)
    with pytest.raises(ValueError):
        DhmmProbSet(-occ - 1, nv, S)


def test_from_arrays_and_to_costs():
    from src.pipeline import DhmmModelSet, DhmmProbSet
    model = R.random_probs([3, 2], 3, 4, seed=61, zeros=0.2)
    p = DhmmProbSet.from_arrays(model.pemit, model.pstay, model.padv, [3, 2])
    assert p.shape == (2, 3, 4) and p.n_states.dtype == np.int32
    costs = p.to_costs()
    assert isinstance(costs, DhmmModelSet)
    want = R.to_costs(model)
    same((costs.emit, costs.stay, costs.adv), (want.emit, want.stay, want.adv), ("emit", "stay", "adv"))
    assert np.isinf(costs.emit).any() and not costs.emit[1, 2].any() and not np.isnan(costs.emit).any()
    for v in (2.0 ** -301, 1.0 + 2.0 ** -52, -0.5, np.nan, np.inf):
        bad = model.pemit.copy()
        bad[0, 0, 0] = v
        with pytest.raises(ValueError):
            DhmmProbSet.from_arrays(bad, model.pstay, model.padv, [3, 2])
    DhmmProbSet.from_arrays(np.full((1, 1, 1), 2.0 ** -300), np.ones((1, 1)), np.zeros((1, 1)), [1])
    with pytest.raises(ValueError):
        DhmmProbSet.from_arrays(model.pemit, model.pstay, model.padv, [3, 4])
    # the Viterbi score of the cost set never exceeds ... the forward likelihood bounds the best path's
    sym, n = D.random_symbols(30, 10, 4, seed=62, lo=3)
    mant, expo, _ = R.forward(model, sym, n)
    vit = D.score(want, sym, n)[0]
    assert (R.nll(mant, expo) <= vit * (1 + 1e-12) + 1e-12).all() and (np.isinf(vit) == (mant == 0)).all()


def test_dhmm_nll():
    from src.pipeline import dhmm_nll
    mant = np.array([[0.5, 0.75, 0.0], [0.999, 0.5, 0.5]])
    expo = np.array([[1, -3000, 0], [0, 1024, -200000]], np.int32)
    got = dhmm_nll(mant, expo)
    same((got,), (R.nll(mant, expo),), ("nll",))
    assert got[0, 0] == 0.0 and np.isinf(got[0, 2]) and got[0, 2] > 0 and got.dtype == np.float64
    assert bits(got[0, 1]) == bits(-(np.log(np.float64(0.75)) + np.float64(-3000) * np.log(np.float64(2.0))))
    assert abs(got[1, 2] - 200001 * np.log(2.0)) < 1e-6


def test_abi_argument_checks():
    """The plan's bounds and the NULL checks, answered on the host before any launch."""
    from src import _hip
    lib = _hip.load_library()
    wb = lib.dsp_dhmm_fb_workspace_bytes
    assert wb(10, 100, 100, 64, 5, 64) > wb(10, 100, 0, 64, 5, 64) > 0 and wb(0, 0, 0, 1, 1, 1) > 0
    assert wb(64, 10000, 10000, 1024, 32, 256) < (1 << 31)  # both budgets bound the workspace
    for args in ((10, 100, 100, 1025, 5, 64), (10, 100, 100, 0, 5, 64), (10, 100, 100, 64, 33, 64), (10, 100, 100, 64, 0, 64),
                 (10, 100, 100, 64, 5, 257), (10, 100, 100, 64, 5, 0), (-1, 100, 100, 64, 5, 64), (10, -1, 100, 64, 5, 64),
                 (10, 100, -1, 64, 5, 64), ((1 << 20) + 1, 100, 100, 64, 5, 64)):
        assert wb(*args) == 0, args
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30

    def forward(C=3, Smax=5, K=64, N=4, T=64, pemit=p, n_states=p, sym=p, outs=(p, p, p), ws=p, nws=big):
        return lib.dsp_dhmm_forward(pemit, p, p, n_states, C, Smax, K, sym, p, N, T, *outs, ws, nws, None)

    def expect(C=3, Smax=5, K=64, N=4, T=64, P=4, pemit=p, start=p, members=p, sym=p, outs=(p, p, p, p, p), ws=p, nws=big):
        return lib.dsp_dhmm_expect(pemit, p, p, p, C, Smax, K, sym, p, N, T, start, members, P, *outs, ws, nws, None)

    for bad in (dict(T=1025), dict(T=0), dict(K=257), dict(K=0), dict(Smax=33), dict(Smax=0), dict(N=-1), dict(C=-1),
                dict(C=(1 << 20) + 1), dict(pemit=None), dict(sym=None)):
        assert forward(**bad) == _hip.DSP_ERR_ARGS, bad
        assert expect(**bad) == _hip.DSP_ERR_ARGS, bad
    assert forward(n_states=None) == _hip.DSP_ERR_ARGS
    for bad in (dict(P=-1), dict(start=None), dict(members=None), dict(outs=(p, p, p, None, p)), dict(outs=(p, p, p, p, None))):
        assert expect(**bad) == _hip.DSP_ERR_ARGS, bad
    assert forward(ws=None, nws=0) == _hip.DSP_ERR_WORKSPACE and forward(nws=wb(3, 4, 0, 64, 5, 64) - 1) == _hip.DSP_ERR_WORKSPACE
    assert expect(ws=None, nws=0) == _hip.DSP_ERR_WORKSPACE and expect(nws=wb(3, 4, 4, 64, 5, 64) - 1) == _hip.DSP_ERR_WORKSPACE
    assert forward(N=0, ws=None, nws=0) == _hip.DSP_OK and forward(outs=(None, None, None), ws=None, nws=0) == _hip.DSP_OK
    assert expect(C=0, ws=None, nws=0) == _hip.DSP_OK
    assert forward(N=0, K=257) == _hip.DSP_ERR_ARGS and expect(C=0, T=0) == _hip.DSP_ERR_ARGS  # the bounds come first


def test_classifier_arguments():
    from src.models import DiscreteHmmClassifier, create_classifier
    clf = DiscreteHmmClassifier()
    assert clf.training == "viterbi" and clf.scoring == "viterbi"
    clf = create_classifier("dhmm", training="baum_welch", scoring="forward", n_iter=3)
    assert clf.training == "baum_welch" and clf.scoring == "forward" and clf.n_iter == 3
    for bad in (dict(training="em"), dict(scoring="sum"), dict(training=None), dict(scoring="Forward")):
        with pytest.raises(ValueError):
            DiscreteHmmClassifier(**bad)
