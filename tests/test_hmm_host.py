"""CPU tests of the HMM definition (tests/hmm_reference.py) and of the host side of the HMM classifier:
the two forms of the restatement agree bit for bit, the score is the minimum over all segmentations,
the seg invariants hold, and the Python surface validates its arguments without a device."""
import ctypes
import itertools

import numpy as np
import pytest

import hmm_reference as H


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def brute_force(x, mu, w, g, stay, adv):
    """The smallest cost over every segmentation of the n frames into S non-empty runs (dyadic values:
    every sum is exact, so the order of the additions does not matter)."""
    n, S = len(x), len(g)
    if n < S:
        return np.inf
    e = np.array([[g[s] + sum(w[s, f] * (x[t, f] - mu[s, f]) ** 2 for f in range(x.shape[1])) for s in range(S)]
                  for t in range(n)])
    best = np.inf
    for cut in itertools.combinations(range(1, n), S - 1):
        b = (0,) + cut + (n,)
        cost = 0.0
        for s in range(S):
            cost += e[b[s]:b[s + 1], s].sum() + (b[s + 1] - b[s] - 1) * stay[s] + (adv[s - 1] if s else 0.0)
        best = min(best, cost)
    return best


def path_cost(x, seg, mu, w, g, stay, adv):
    """The recurrence's own additions along a given segmentation."""
    S, n = len(g), len(x)
    state = np.searchsorted(np.asarray(seg), np.arange(n), side="right") - 1
    v = None
    for t in range(n):
        s = state[t]
        e = g[s]
        for f in range(x.shape[1]):
            d = x[t, f] - mu[s, f]
            e = e + w[s, f] * (d * d)
        v = e if t == 0 else e + (v + (stay[s] if state[t - 1] == s else adv[s - 1]))
    return v


def check_seg(seg, S, n, Smax):
    assert seg[0] == 0 and (np.diff(seg[:S]) > 0).all() and seg[S - 1] < n and (seg[S:] == -1).all()
    assert len(seg) == Smax


@pytest.mark.parametrize("F", (1, 2))
def test_score_is_the_minimum_over_all_segmentations(F):
    """400 dyadic cases with n <= 9, S <= 5: the table form's score is the brute force's, every n < S
    gives +inf, and at F = 1 a fifth of the finite pairs meet an exact tie on the way back."""
    model = H.dyadic_models(20, 5, F, seed=1)
    x, n = H.dyadic_sequences(20, 9, F, seed=2)
    finite = short = 0
    for c in range(20):
        m = model.one(c)
        for i in range(20):
            xi = x[i, :n[i]]
            sc, seg = H.viterbi_table(xi, *m)
            want = brute_force(xi, *m)
            assert sc == want, (c, i, sc, want)
            if n[i] < model.n_states[c]:
                assert sc == np.inf and seg is None
                short += 1
            else:
                assert np.isfinite(sc)
                check_seg(np.array(seg), len(seg), n[i], len(seg))
                assert bits(path_cost(xi, seg, *m)) == bits(sc)
                finite += 1
    assert finite > 250 and short > 50
    frac, count = H.tie_fraction(model, x, n)
    assert count == finite and (frac >= 0.2 or F > 1), frac


@pytest.mark.parametrize("F", (1, 2, 3, 8))
def test_the_two_forms_agree(F):
    """Random reals and the dyadic corpus, mixed n_states with Smax = 32, lengths 1 .. 40 and invalid
    ones, a CSR list with an empty group, a repeated sequence and out-of-range members."""
    S = [1, 2, 5, 31, 32, 3, 32, 1, 7, 0, 33]
    N, T = 23, 40
    rng = np.random.default_rng(10 + F)
    for model, (x, n) in ((H.random_models(S, 32, F, seed=F), (rng.normal(0, 1, (N, T, F)), rng.integers(1, T + 1, N).astype(np.int32))),
                          (H.dyadic_models(11, 32, F, seed=F, n_states=S), H.dyadic_sequences(N, T, F, seed=20 + F))):
        n[[3, 4]] = [0, T + 1]
        n[[5, 6, 7]] = [31, 32, 33]
        groups = [list(rng.integers(0, N, k)) for k in (3, 0, 5, 23, 9, 2, 4, 1, 6, 3, 3)]
        groups[2] += [-1, N, 7, 7]
        start = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
        members = np.array([r for g in groups for r in g], np.int32)
        sa, ga = H.align(model, x, n, start, members, "table")
        sb, gb = H.align(model, x, n, start, members, "rows")
        assert np.array_equal(bits(sa), bits(sb)) and np.array_equal(ga, gb)
        owner = np.repeat(np.arange(11), np.diff(start))
        for p, (c, k) in enumerate(zip(owner, members)):
            Sc = S[c]
            bad = not (0 <= k < N) or not (1 <= n[k] <= T) or not (1 <= Sc <= 32)
            if bad or n[k] < Sc:
                assert sa[p] == np.inf and (ga[p] == -1).all()
            else:
                assert np.isfinite(sa[p])
                check_seg(ga[p], Sc, n[k], 32)
                assert bits(path_cost(x[k, :n[k]], ga[p, :Sc], *model.one(c))) == bits(sa[p])
        full_a, lab_a = H.score(model, x, n, "table")
        full_b, lab_b = H.score(model, x, n, "rows")
        assert np.array_equal(bits(full_a), bits(full_b)) and np.array_equal(lab_a, lab_b)
        ok = (members >= 0) & (members < N)
        assert np.array_equal(bits(sa[ok]), bits(full_a[members[ok], owner[ok]]))
        assert (lab_a[[3, 4]] == -1).all() and (lab_a[n >= 1][n[n >= 1] <= T] >= 0).all()


def test_infinite_costs_give_no_nan():
    model = H.random_models([5, 5], 5, 2, seed=3)
    model.stay[0, 2], model.adv[0, 1], model.adv[1, 3] = np.inf, np.inf, np.inf
    x = np.random.default_rng(4).normal(0, 1, (6, 12, 2))
    n = np.array([5, 6, 12, 9, 4, 12], np.int32)
    sc, lab = H.score(model, x, n, "table")
    assert not np.isnan(sc).any() and np.array_equal(bits(sc), bits(H.score(model, x, n, "rows")[0]))
    assert np.isinf(sc).all() and (lab == -1).all()  # no path passes an infinite advance
    model.adv[0, 1] = model.adv[1, 3] = 1.0
    sc = H.score(model, x, n, "table")[0]
    assert np.isfinite(sc[n >= 5]).all() and np.isinf(sc[4]).all() and not np.isnan(sc).any()
    seg = H.align(model, x, n, [0, 6, 6], np.arange(6), "table")[1]
    assert (seg[n >= 5, 3] - seg[n >= 5, 2] == 1).all()  # stay = +inf: state 2 holds one frame


def test_accumulate_and_model_build():
    """The reference accumulate against plain sums, the copy rule, the variance floor, and the host
    build of pipeline.HmmModelSet against the state-by-state restatement, bit for bit."""
    from src.pipeline import HmmModelSet, hmm_uniform_segmentation
    rng = np.random.default_rng(5)
    N, T, F, S = 40, 30, 3, [4, 1, 6, 5]
    x, n = rng.normal(0, 1, (N, T, F)), rng.integers(3, T + 1, N).astype(np.int32)
    x[:, :, 2] = 1.5  # a constant channel: its variance hits the floor
    codes = np.arange(N) % 3  # model 3 has no member
    order = np.argsort(codes, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=4))])
    pair_states = np.array(S)[codes[order]]
    seg = H.uniform_seg(n[order], pair_states, 6)
    assert np.array_equal(seg, hmm_uniform_segmentation(n[order], pair_states, 6))
    assert (seg[n[order] < pair_states] == -1).all() and (n[order] < pair_states).any()
    prev_mu, prev_var = rng.normal(0, 1, (4, 6, F)), rng.uniform(1, 2, (4, 6, F))
    mean, var, cnt, n_valid, total = H.accumulate(prev_mu, prev_var, S, x, n, start, order, seg, np.ones(N), 1e-3)
    assert n_valid.tolist() == [int((n[codes == c] >= S[c]).sum()) for c in range(3)] + [0]
    assert np.array_equal(bits(mean[3]), bits(prev_mu[3])) and np.array_equal(bits(var[3]), bits(prev_var[3]))
    assert total.tolist() == [float(v) for v in n_valid] and not cnt[3].any()
    assert (var[:3, :, 2][np.arange(6)[None, :] < np.array(S[:3])[:, None]] == 1e-3).all()
    assert cnt[1, 0] == n[codes == 1].sum() and np.allclose(mean[1, 0], x[codes == 1][np.arange(T)[None, :] < n[codes == 1][:, None]].mean(axis=0))
    assert not mean[0, 4:].any() and not var[1, 1:].any() and not cnt[0, 4:].any()
    want = H.build_model(mean, var, cnt, n_valid, S, 1e-3)
    got = HmmModelSet(mean, var, cnt, n_valid, S, 1e-3)
    for name in ("w", "g", "stay", "adv"):
        assert np.array_equal(bits(getattr(got, name)), bits(getattr(want, name))), name
    assert np.array_equal(bits(got.mean), bits(want.mu)) and np.array_equal(got.n_states, want.n_states)
    assert got.stay[3, 0] == -np.log(0.5) and got.stay[1, 0] == -np.log((cnt[1, 0] - n_valid[1]) / cnt[1, 0])
    again = HmmModelSet(mean, var, cnt, n_valid, S, 1e-3, prev=want)
    assert np.array_equal(bits(again.stay), bits(H.build_model(mean, var, cnt, n_valid, S, 1e-3, prev=want).stay))


def test_create_classifier_validates_without_a_device():
    from src.models import HmmClassifier, SequenceClassifier, create_classifier
    clf = create_classifier('hmm')
    assert isinstance(clf, HmmClassifier) and isinstance(clf, SequenceClassifier)
    assert (clf.n_states, clf.n_iter, clf.var_floor, clf.trans_floor, clf.normalize) == (5, 10, 1e-3, 1e-3, True)
    assert create_classifier('hmm', n_states=[3, 32, 1]).n_states.tolist() == [3, 32, 1]
    for bad in (dict(n_states=0), dict(n_states=33), dict(n_states=[3, 40]), dict(n_states=2.5), dict(n_iter=-1),
                dict(var_floor=0.0), dict(trans_floor=0.5), dict(trans_floor=0.0), dict(n_states=[])):
        with pytest.raises(ValueError):
            create_classifier('hmm', **bad)
    for name in ("fit", "predict", "score_samples", "evaluate"):
        assert callable(getattr(clf, name))


def test_abi_argument_checks():
    """The plan's bounds and the NULL checks, answered on the host before any launch."""
    from src import _hip
    lib = _hip.load_library()
    wb = lib.dsp_hmm_workspace_bytes
    assert wb(10, 100, 100, 64, 2, 5) > 0 and wb(10, 100, 0, 1024, 8, 32) > 0
    for args in ((10, 100, 100, 1025, 2, 5), (10, 100, 100, 64, 9, 5), (10, 100, 100, 64, 0, 5), (10, 100, 100, 64, 2, 33),
                 (10, 100, 100, 64, 2, 0), (-1, 100, 100, 64, 2, 5), (10, 100, 100, 0, 2, 5)):
        assert wb(*args) == 0, args
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    model = (p, p, p, p, p, p, 3, 5)
    assert lib.dsp_hmm_score(*model, p, p, 4, 64, 9, p, p, p, 1 << 30, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_hmm_score(*model[:6], 3, 33, p, p, 4, 64, 2, p, p, p, 1 << 30, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_hmm_score(*model, None, p, 4, 64, 2, p, p, p, 1 << 30, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_hmm_score(*model, p, p, 4, 64, 2, p, p, None, 0, None) == _hip.DSP_ERR_WORKSPACE
    assert lib.dsp_hmm_score(*model, p, p, 0, 64, 2, p, p, None, 0, None) == _hip.DSP_OK
    assert lib.dsp_hmm_score(*model, p, p, 4, 64, 2, None, None, None, 0, None) == _hip.DSP_OK
    assert lib.dsp_hmm_align(*model, p, p, 4, 1025, 2, p, p, 4, p, p, p, 1 << 30, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_hmm_align(*model, p, p, 4, 64, 2, None, p, 4, p, p, p, 1 << 30, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_hmm_align(*model, p, p, 4, 64, 2, p, p, 4, p, p, p, 8, None) == _hip.DSP_ERR_WORKSPACE
    assert lib.dsp_hmm_align(*model, p, p, 4, 64, 2, p, p, 0, p, p, None, 0, None) == _hip.DSP_OK
    q, q2 = ctypes.c_void_p(p.value + 8), ctypes.c_void_p(p.value + 16)
    acc = lambda mean, ws, nws, C=3: lib.dsp_hmm_accumulate(p, p, p, C, 5, p, p, 4, 64, 2, p, p, 4, p, p, 1e-3, mean, q2, p, p, p,
                                                           ws, nws, None)
    assert acc(None, p, 1 << 30) == _hip.DSP_ERR_ARGS and acc(p, p, 1 << 30) == _hip.DSP_ERR_ARGS  # mean == mu_prev
    assert acc(q, None, 0) == _hip.DSP_ERR_WORKSPACE and acc(q, None, 0, C=0) == _hip.DSP_OK


ALIGN_WORKSPACE = {  # dsp_dtw_align_workspace_bytes(Na, P, Ta, Tb, F); a pair chunk at Ta = 1024, F = 8 is 1820 pairs
    (19, 0, 70, 70, 3): 2789632,
    (19, 37, 70, 70, 3): 2870272,
    (1, 1, 1, 1, 1): 2816,
    (3, 100, 1, 1024, 1): 4198656,
    (3, 100, 1024, 1, 1): 1744640,
    (10, 1819, 1024, 1024, 8): 792586496,
    (10, 1820, 1024, 1024, 8): 792660224,
    (10, 1821, 1024, 1024, 8): 792660224,
    (10, 8000, 1024, 1024, 8): 1207896320,
    (1024, 5000, 33, 40, 2): 73042944,
    (1025, 5000, 33, 40, 2): 73042944,
    (5000, 300000, 33, 40, 2): 388566528,
    (10 ** 9, (1 << 31) - 1, 1024, 1024, 8): 1309653248,
}
HMM_WORKSPACE = {  # dsp_hmm_workspace_bytes(C, N, P, T, F, Smax); a pair chunk at Smax = 32, F = 8 is 31 775 pairs
    (0, 0, 0, 1, 1, 1): 1024,
    (10, 100, 0, 64, 2, 5): 191232,
    (10, 100, 100, 64, 2, 5): 225280,
    (1, 1, 1, 1, 1, 1): 2816,
    (3, 10, 100, 1024, 8, 32): 1488896,
    (2, 6, 31774, 3, 8, 32): 134607872,
    (2, 6, 31775, 3, 8, 32): 134612224,
    (2, 6, 31776, 3, 8, 32): 134612224,
    (2, 6, 31800, 3, 8, 32): 134612224,
    (1024, 50, 5000, 8, 2, 4): 5254400,
    (1025, 50, 5000, 8, 2, 4): 5256960,
    (5000, 321, 300000, 8, 2, 4): 73548800,
    (1 << 20, 1000, (1 << 31) - 2, 1024, 8, 32): 14965276672,
}


def test_workspace_sizes_are_recorded():
    """The two pair-list workspaces byte for byte (the layouts behind them are part of what a caller
    allocates once and keeps): P = 0, either side of a pair chunk, 1024 and 1025 groups, T = 1 and 1024,
    and the largest shapes of the plans.  The values are those of the library before csrc/csr_pairs.h."""
    from src import _hip
    lib = _hip.load_library()
    for args, want in ALIGN_WORKSPACE.items():
        assert lib.dsp_dtw_align_workspace_bytes(*args) == want, args
    for args, want in HMM_WORKSPACE.items():
        assert lib.dsp_hmm_workspace_bytes(*args) == want, args
