"""GPU tests of csrc/hmm.hip (dsp_hmm_score, dsp_hmm_align, dsp_hmm_accumulate) through the bare C ABI,
and of the Python surface on it.  Everything is compared with the numpy restatement of
tests/hmm_reference.py on the raw bits and the raw integers: scores, state paths and re-estimated
models are defined bit for bit, so there is no tolerance and no pair is left out."""
import functools
import wave

import numpy as np
import pytest

import hmm_reference as H
from device_outputs import Guarded, _dev, bits, csr

pytestmark = pytest.mark.gpu

STATES = [1, 2, 5, 31, 32, 3, 32, 1, 7, 2, 5]  # C = 11, mixed within one model set


def _nan_after(x):
    """A float64 input followed by NaN: a read past its end would poison a result."""
    import torch
    return _dev(np.concatenate([np.asarray(x, np.float64).reshape(-1), np.full(64, np.nan)]), torch.float64)


def _model_args(model):
    import torch
    from src import _hip
    keep = [_nan_after(a) for a in (model.mu, model.w, model.g, model.stay, model.adv)]
    keep.append(_dev(np.concatenate([model.n_states, np.full(16, 1 << 20, np.int32)]), torch.int32))
    C, Smax = model.mu.shape[:2]
    return keep, [_hip.ptr(t) for t in keep] + [C, Smax]


def _workspace(C, N, P, T, F, Smax):
    import torch
    from src import _hip
    nbytes = _hip.lib().dsp_hmm_workspace_bytes(C, N, P, T, F, Smax)
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes


def score_raw(model, x, n, with_score=True, with_label=True):
    """dsp_hmm_score through the bare C ABI -> (score, label), None where not asked for."""
    import torch
    from src import _hip
    N, T, F = x.shape
    keep, margs = _model_args(model)
    C, Smax = margs[-2:]
    tx, tn = _nan_after(x), _dev(np.asarray(n, np.int32), torch.int32)
    gs, gl = Guarded((N, C), torch.float64, -7.0), Guarded((N,), torch.int32, -9)
    ws, nbytes = _workspace(C, N, 0, T, F, Smax)
    rc = _hip.lib().dsp_hmm_score(*margs, _hip.ptr(tx), _hip.ptr(tn), N, T, F, _hip.ptr(gs.view) if with_score else None,
                                  _hip.ptr(gl.view) if with_label else None, _hip.ptr(ws), nbytes, _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    score, label = gs.get(), gl.get()
    if not with_score:
        assert (score == -7.0).all()
        score = None
    if not with_label:
        assert (label == -9).all()
        label = None
    return score, label


def align_raw(model, x, n, start, members, with_score=True, with_seg=True):
    """dsp_hmm_align through the bare C ABI -> (score, seg), None where not asked for."""
    import torch
    from src import _hip
    N, T, F = x.shape
    keep, margs = _model_args(model)
    C, Smax = margs[-2:]
    P = len(members)
    tx, tn = _nan_after(x), _dev(np.asarray(n, np.int32), torch.int32)
    ts = _dev(np.asarray(start, np.int32), torch.int32)
    tm = _dev(np.concatenate([np.asarray(members, np.int32), np.full(16, 1 << 20, np.int32)]), torch.int32)
    gs, gg = Guarded((P,), torch.float64, -7.0), Guarded((P, Smax), torch.int32, -9)
    ws, nbytes = _workspace(C, N, P, T, F, Smax)
    rc = _hip.lib().dsp_hmm_align(*margs, _hip.ptr(tx), _hip.ptr(tn), N, T, F, _hip.ptr(ts), _hip.ptr(tm), P,
                                  _hip.ptr(gs.view) if with_score else None, _hip.ptr(gg.view) if with_seg else None,
                                  _hip.ptr(ws), nbytes, _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    score, seg = gs.get(), gg.get()
    if not with_score:
        assert (score == -7.0).all()
        score = None
    if not with_seg:
        assert (seg == -9).all()
        seg = None
    return score, seg


def accumulate_raw(mu_prev, var_prev, n_states, x, n, start, members, seg, score, var_floor):
    """dsp_hmm_accumulate through the bare C ABI -> (mean, var, cnt, n_valid, total)."""
    import torch
    from src import _hip
    N, T, F = x.shape
    C, Smax = mu_prev.shape[:2]
    P = len(members)
    tin = [_nan_after(mu_prev), _nan_after(var_prev), _dev(np.asarray(n_states, np.int32), torch.int32), _nan_after(x),
           _dev(np.asarray(n, np.int32), torch.int32), _dev(np.asarray(start, np.int32), torch.int32),
           _dev(np.concatenate([np.asarray(members, np.int32), np.full(16, 1 << 20, np.int32)]), torch.int32),
           _dev(np.concatenate([np.asarray(seg, np.int32).reshape(-1), np.full(64, 1 << 20, np.int32)]), torch.int32),
           _nan_after(score)]
    out = [Guarded((C, Smax, F), torch.float64, -7.0), Guarded((C, Smax, F), torch.float64, -7.0),
           Guarded((C, Smax), torch.int32, -9), Guarded((C,), torch.int32, -9), Guarded((C,), torch.float64, -7.0)]
    ws, nbytes = _workspace(C, N, P, T, F, Smax)
    p = [_hip.ptr(t) for t in tin]
    rc = _hip.lib().dsp_hmm_accumulate(p[0], p[1], p[2], C, Smax, p[3], p[4], N, T, F, p[5], p[6], P, p[7], p[8],
                                       float(var_floor), *[_hip.ptr(o.view) for o in out], _hip.ptr(ws), nbytes,
                                       _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    return tuple(o.get() for o in out)


def same_bits(got, want):
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]


@functools.lru_cache(maxsize=None)
def table_case(F):
    """C = 11 models of 1 .. 32 states against 130 sequences of T = 65: random reals, lengths covering
    1, S-1, S, S+1 of every model, 31, 32, 33 and 65; NaN behind each sequence's frames."""
    model = H.random_models(STATES, 32, F, seed=40 + F)
    rng = np.random.default_rng(50 + F)
    N, T = 130, 65
    x, n = rng.normal(0, 1, (N, T, F)), rng.integers(1, T + 1, N).astype(np.int32)
    edge = [1, 2, 3, 4, 5, 6, 7, 8, 30, 31, 32, 33, 65, 65, 1]
    n[:len(edge)] = edge
    n[60:60 + len(edge)] = edge  # the same lengths in lanes of the next wave
    x[np.arange(T)[None, :] >= n[:, None]] = np.nan
    want = H.score(model, np.nan_to_num(x), n)
    return model, x, n, want


@pytest.mark.parametrize("F", (1, 2, 3, 8))
def test_score_table(F):
    model, x, n, (ws, wl) = table_case(F)
    assert np.isinf(ws).any() and np.isfinite(ws).sum() > 1000 and not np.isnan(ws).any()
    score, label = score_raw(model, x, n)
    same_bits(score, ws)
    assert np.array_equal(label, wl) and (label >= 0).all()
    only_s = score_raw(model, x, n, with_label=False)
    only_l = score_raw(model, x, n, with_score=False)
    same_bits(only_s[0], ws)
    assert only_s[1] is None and only_l[0] is None and np.array_equal(only_l[1], wl)


@pytest.mark.parametrize("N", (1, 63, 64, 65))
def test_score_partial_and_multiple_tiles(N):
    """The first N sequences alone (a partial wave, a full one, a second tile), and C = 1."""
    model, x, n, (ws, wl) = table_case(2)
    score, label = score_raw(model, x[:N], n[:N])
    same_bits(score, ws[:N])
    assert np.array_equal(label, wl[:N])
    one = H.Model(model.mu[4:5], model.w[4:5], model.g[4:5], model.stay[4:5], model.adv[4:5], [32])
    score, label = score_raw(one, x[:N], n[:N])
    same_bits(score[:, 0], ws[:N, 4])
    assert np.array_equal(label, np.where(np.isinf(ws[:N, 4]), -1, 0))


def table_groups(rng, N):
    """Groups of 1, 63, 64, 65, 130 and 0 members and five more; sequence 7 under two models."""
    groups = [rng.integers(0, N, k).tolist() for k in (1, 63, 64, 65, 130, 0, 17, 40, 5, 70, 3)]
    groups[0] = [7]
    groups[8].append(7)
    return groups


@pytest.mark.parametrize("F", (1, 2, 3, 8))
def test_align_table(F):
    model, x, n, (full, _) = table_case(F)
    start, members = csr(table_groups(np.random.default_rng(60 + F), len(x)))
    ws, wg = H.align(model, np.nan_to_num(x), n, start, members)
    owner = np.repeat(np.arange(11), np.diff(start))
    same_bits(ws, full[members, owner])
    assert start[5] == start[6] and (members == 7).sum() >= 2 and np.isfinite(ws).sum() > 200
    score, seg = align_raw(model, x, n, start, members)
    same_bits(score, ws)
    assert np.array_equal(seg, wg), np.argwhere(seg != wg)[:5]
    for p in np.flatnonzero(np.isfinite(score)):  # the invariants, from the device's own output alone
        S = STATES[owner[p]]
        assert seg[p, 0] == 0 and (np.diff(seg[p, :S]) > 0).all() and seg[p, S - 1] < n[members[p]] and (seg[p, S:] == -1).all()
    assert (seg[np.isinf(score)] == -1).all()
    only_s = align_raw(model, x, n, start, members, with_seg=False)
    only_g = align_raw(model, x, n, start, members, with_score=False)
    same_bits(only_s[0], ws)
    assert only_s[1] is None and only_g[0] is None and np.array_equal(only_g[1], wg)


def test_invalid_input():
    """Lengths 0 and T + 1, n_states 0 and 33, members -1 and N, an empty group, one sequence under two
    models: +inf and -1 there, the restatement's values everywhere else; P = 0 writes nothing."""
    model, x, n, _ = table_case(2)
    x, n = x.copy(), n.copy()
    n[[20, 21]] = [0, 66]
    states = np.array(STATES)
    states[[2, 9]] = [0, 33]
    bad = H.Model(model.mu, model.w, model.g, model.stay, model.adv, states)
    ws, wl = H.score(bad, np.nan_to_num(x), n)
    assert np.isinf(ws[[20, 21]]).all() and np.isinf(ws[:, [2, 9]]).all() and (wl[[20, 21]] == -1).all()
    score, label = score_raw(bad, x, n)
    same_bits(score, ws)
    assert np.array_equal(label, wl)
    groups = table_groups(np.random.default_rng(70), len(x))
    groups[3] += [-1, len(x), 20, 21, 1 << 30, -(1 << 31)]
    start, members = csr(groups)
    wa, wg = H.align(bad, np.nan_to_num(x), n, start, members)
    assert np.isinf(wa).sum() >= 6 + len(groups[2]) + len(groups[9]) and np.isfinite(wa).sum() > 100
    score, seg = align_raw(bad, x, n, start, members)
    same_bits(score, wa)
    assert np.array_equal(seg, wg) and (seg[np.isinf(score)] == -1).all()
    score, seg = align_raw(bad, x, n, np.zeros(12, np.int32), np.zeros(0, np.int32))
    assert score.shape == (0,) and seg.shape == (0, 32)


def test_tie_rule():
    """The dyadic corpus (integer data and means, w = 0.5, g in {0, 1}, stay / adv in {0, 0.5, 1}) at
    N = 130, C = 11: at least a fifth of the finite pairs meet a finite tie a == b on the way back, so
    the strict < decides their paths."""
    model = H.dyadic_models(11, 32, 1, seed=3, n_states=STATES)
    x, n = H.dyadic_sequences(130, 65, 1, seed=4)
    frac, finite = H.tie_fraction(model, x, n)
    assert frac >= 0.2 and finite > 1000, (frac, finite)
    start, members = csr([list(range(130))] * 11)
    ws, wg = H.align(model, x, n, start, members)
    score, seg = align_raw(model, x, n, start, members)
    same_bits(score, ws)
    assert np.array_equal(seg, wg), np.argwhere(seg != wg)[:5]
    same_bits(score_raw(model, x, n)[0], ws.reshape(11, 130).T)


def test_infinite_costs():
    """stay = +inf on one state (it holds one frame) and adv = +inf on another (nothing passes): no NaN."""
    model = H.random_models([5, 5, 32], 32, 2, seed=80)
    model.stay[0, 2], model.adv[1, 3], model.stay[2, 30], model.g[2, 5] = np.inf, np.inf, np.inf, np.inf
    rng = np.random.default_rng(81)
    x, n = rng.normal(0, 1, (70, 40, 2)), rng.integers(1, 41, 70).astype(np.int32)
    start, members = csr([list(range(70))] * 3)
    ws, wg = H.align(model, x, n, start, members)
    assert not np.isnan(ws).any() and np.isinf(ws[70:]).all() and np.isfinite(ws[:70][n >= 5]).all()
    score, seg = align_raw(model, x, n, start, members)
    same_bits(score, ws)
    assert np.array_equal(seg, wg)
    same_bits(score_raw(model, x, n)[0], ws.reshape(3, 70).T)


def test_longest_sequences():
    """One tile at T = 1024 with S = 32 (and S = 1): lengths 1024, 1000, 32, 31 and 1."""
    model = H.random_models([32, 1], 32, 2, seed=90)
    rng = np.random.default_rng(91)
    x, n = rng.normal(0, 1, (5, 1024, 2)), np.array([1024, 1000, 32, 31, 1], np.int32)
    start, members = csr([[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]])
    ws, wg = H.align(model, x, n, start, members)
    assert np.isfinite(ws[[0, 1, 2]]).all() and np.isinf(ws[[3, 4]]).all() and np.isfinite(ws[5:]).all()
    score, seg = align_raw(model, x, n, start, members)
    same_bits(score, ws)
    assert np.array_equal(seg, wg) and seg[0, 31] > seg[0, 1] > 0
    same_bits(score_raw(model, x, n)[0], np.stack([ws[:5], ws[5:][::-1]], axis=1))


def test_more_tiles_than_waves():
    """C = 1030 models (two launches of at most 1024) against 321 sequences (six tiles per model): 6144
    tiles for 4096 persistent waves, so a wave takes a second tile; short sequences, S <= 4."""
    rng = np.random.default_rng(100)
    C, N, T, F = 1030, 321, 8, 2
    states = rng.integers(1, 5, C)
    model = H.random_models(states, 4, F, seed=101)
    x, n = rng.normal(0, 1, (N, T, F)), rng.integers(1, T + 1, N).astype(np.int32)
    ws, wl = H.score(model, x, n)
    score, label = score_raw(model, x, n)
    same_bits(score, ws)
    assert np.array_equal(label, wl)
    start, members = csr([list(range(N))] * C)
    wa, wg = H.align(model, x, n, start, members)
    same_bits(wa, ws.T.reshape(-1))
    score, seg = align_raw(model, x, n, start, members)
    same_bits(score, wa)
    assert np.array_equal(seg, wg)


def test_labels():
    """An all-+inf row gives -1; two identical models tie exactly and the smaller index wins."""
    base = H.random_models([3, 4, 6], 6, 2, seed=110)
    pick = [2, 1, 0, 1, 2]  # models 1 and 3, 0 and 4 are identical
    model = H.Model(base.mu[pick], base.w[pick], base.g[pick], base.stay[pick], base.adv[pick], base.n_states[pick])
    rng = np.random.default_rng(111)
    x, n = rng.normal(0, 1, (40, 12, 2)), rng.integers(3, 13, 40).astype(np.int32)
    n[:3] = [1, 2, 2]
    ws, wl = H.score(model, x, n)
    score, label = score_raw(model, x, n)
    same_bits(score, ws)
    assert np.array_equal(label, wl) and (label[:3] == -1).all() and np.isinf(score[:3]).all()
    same_bits(score[:, 1], score[:, 3])
    same_bits(score[:, 0], score[:, 4])
    assert set(label[3:].tolist()) <= {0, 1, 2} and (label[3:] == np.argmin(score[3:], axis=1)).all()
    assert len(set(label[3:].tolist())) > 1


def accumulate_case(seed=120):
    """Five models (S = 4, 1, 6, 5, 3) over 90 sequences, random reals: groups of 40, 16, 17, 0 and 5
    members in a shuffled order; a constant channel (its variance hits the floor); model 3 has no
    member and model 4 only members that are skipped."""
    rng = np.random.default_rng(seed)
    N, T, F, S = 90, 30, 3, np.array([4, 1, 6, 5, 3])
    x, n = rng.normal(0, 1, (N, T, F)) * [1.0, 30.0, 1.0], rng.integers(6, T + 1, N).astype(np.int32)
    x[:, :, 2] = 1.5
    n[80:] = 2
    groups = [rng.permutation(80)[:k].tolist() for k in (40, 16, 17, 0)] + [[80, 81, -1, N, 82]]
    start, members = csr(groups)
    mu_prev, var_prev = rng.normal(0, 1, (5, 6, F)), rng.uniform(1, 2, (5, 6, F))
    return x, n, S, start, members, mu_prev, var_prev


def check_accumulate(got, want):
    for g, w, name in zip(got, want, ("mean", "var", "cnt", "n_valid", "total")):
        if g.dtype == np.float64:
            assert np.array_equal(bits(g), bits(w)), (name, np.argwhere(bits(g) != bits(w))[:5])
        else:
            assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


def test_accumulate():
    x, n, S, start, members, mu_prev, var_prev = accumulate_case()
    owner = np.repeat(np.arange(5), np.diff(start))
    ok = (members >= 0) & (members < len(x))
    lengths = np.where(ok, n[np.where(ok, members, 0)], 0)
    seg = H.uniform_seg(lengths, S[owner], 6)
    score = np.random.default_rng(121).uniform(1, 100, len(members))
    want = H.accumulate(mu_prev, var_prev, S, x, n, start, members, seg, score, 1e-3)
    assert want[3].tolist() == [40, 16, 17, 0, 0] and (want[1][0, :4, 2] == 1e-3).all()
    assert np.array_equal(bits(want[0][3:]), bits(mu_prev[3:])) and want[4][3:].tolist() == [0.0, 0.0]
    check_accumulate(accumulate_raw(mu_prev, var_prev, S, x, n, start, members, seg, score, 1e-3), want)
    # the order of the list is the order of the sums
    swapped = members.copy()
    swapped[:40] = swapped[:40][::-1]
    other = H.accumulate(mu_prev, var_prev, S, x, n, start, swapped, seg[np.r_[39:-1:-1, 40:len(members)]], score, 1e-3)
    assert not np.array_equal(bits(other[0][0]), bits(want[0][0]))
    check_accumulate(accumulate_raw(mu_prev, var_prev, S, x, n, start, swapped, seg[np.r_[39:-1:-1, 40:len(members)]],
                                    score, 1e-3), other)
    # malformed seg rows are skipped: not starting at 0, not increasing, past the end, an n_states of 0
    seg2 = seg.copy()
    seg2[0, 0], seg2[1, 2], seg2[2, 3] = 1, seg2[1, 1], 1000
    S2 = S.copy()
    S2[1] = 0
    want2 = H.accumulate(mu_prev, var_prev, S2, x, n, start, members, seg2, score, 1e-3)
    assert want2[3].tolist() == [37, 0, 17, 0, 0]
    check_accumulate(accumulate_raw(mu_prev, var_prev, S2, x, n, start, members, seg2, score, 1e-3), want2)


def test_accumulate_after_align():
    """dsp_hmm_align's own seg and score as the input, F = 2 and S up to 32."""
    model, x, n, _ = table_case(2)
    x = np.nan_to_num(x)
    start, members = csr(table_groups(np.random.default_rng(130), len(x)))
    score, seg = align_raw(model, x, n, start, members)
    want = H.accumulate(model.mu, model.var, STATES, x, n, start, members, seg, score, 1e-3)
    assert want[3][5] == 0 and want[3][4] > 50
    check_accumulate(accumulate_raw(model.mu, model.var, STATES, x, n, start, members, seg, score, 1e-3), want)


def test_accumulate_pair_chunks():
    """More pairs than one pair chunk holds: at Smax = 32, F = 8 the plan sums 128 MiB / (32 (4 + 16 * 8))
    = 31 775 pairs per chunk, and 31 800 pairs over two models (S = 1, 2) put the chunk boundary inside
    the second group, 11 775 = 16 * 735 + 15 pairs behind its start.  cnt, n_valid, total and both sums
    are carried across it.  Six sequences of 1 .. 3 frames reused through members; members -1 and N and
    the one-frame sequences under the two-state model are skipped, on both sides of the boundary."""
    Smax, F, T, N = 32, 8, 3, 6
    chunk = (128 << 20) // (Smax * (4 + 16 * F))
    sizes = [20000, 11800]
    P = sum(sizes)
    assert chunk == 31775 and P > chunk and sizes[0] < chunk and (chunk - sizes[0]) % 16 == 15
    rng = np.random.default_rng(160)
    x, n = rng.normal(0, 1, (N, T, F)), np.array([3, 1, 2, 3, 2, 1], np.int32)
    S = np.array([1, 2])
    members = rng.integers(0, N, P).astype(np.int32)
    members[rng.choice(P, 40, replace=False)] = np.tile([-1, N], 20)
    members[[chunk - 2, chunk + 1]] = [N, -1]
    members[[chunk - 1, chunk]] = [0, 3]  # valid members on either side of the boundary
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    owner = np.repeat(np.arange(2), sizes)
    ok = (members >= 0) & (members < N)
    seg = H.uniform_seg(np.where(ok, n[np.where(ok, members, 0)], 0), S[owner], Smax)
    score = rng.uniform(1, 100, P)
    mu_prev, var_prev = rng.normal(0, 1, (2, Smax, F)), rng.uniform(1, 2, (2, Smax, F))
    want = H.accumulate(mu_prev, var_prev, S, x, n, start, members, seg, score, 1e-3)
    short = int((ok & (n[np.where(ok, members, 0)] < 2))[sizes[0]:].sum())
    assert want[3][0] == int(ok[:sizes[0]].sum()) < sizes[0]
    assert want[3][1] == int(ok[sizes[0]:].sum()) - short and short > 1000
    check_accumulate(accumulate_raw(mu_prev, var_prev, S, x, n, start, members, seg, score, 1e-3), want)


def word_sequences(seed, per_class=20):
    """3 classes x 20 sequences of 12 .. 40 frames, F = 2, drawn from known left-to-right models; the
    classes interleaved, labels 2, 7, 12."""
    rng = np.random.default_rng(seed)
    means = np.random.default_rng(7).normal(0, 2.0, (3, 5, 2)) * [1.0, 40.0]
    seqs, y = [], []
    for i in range(3 * per_class):
        c, n = i % 3, int(rng.integers(12, 41))
        cuts = np.sort(rng.choice(np.arange(1, n), 4, replace=False))
        state = np.searchsorted(cuts, np.arange(n), side="right")
        seqs.append(means[c, state] + rng.normal(0, 0.5, (n, 2)) * [1.0, 40.0])
        y.append(5 * c + 2)
    return seqs, np.array(y)


def pad(seqs):
    n = np.array([len(s) for s in seqs], np.int32)
    out = np.zeros((len(seqs), int(n.max()), seqs[0].shape[1]))
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out, n


def test_hmm_classifier():
    from src.models import create_classifier
    from src.pipeline import hmm_align, hmm_score
    seqs, y = word_sequences(140)
    clf = create_classifier('hmm', n_states=[5, 4, 6], n_iter=6).fit(seqs, y)
    frames = np.concatenate(seqs)
    mean, std = frames.mean(axis=0), frames.std(axis=0)
    X, n = pad([(s - mean) / std for s in seqs])
    classes, codes = np.unique(y, return_inverse=True)
    model, totals = H.fit(X, n, codes, [5, 4, 6], n_iter=6)
    assert 1 <= len(totals) <= 6 and clf.totals_.shape == totals.shape and clf.n_iter_ == len(totals)
    same_bits(clf.totals_, totals)
    for name in ("w", "g", "stay", "adv"):
        same_bits(getattr(clf.model_, name), getattr(model, name))
    same_bits(clf.model_.mean, model.mu)
    same_bits(clf.model_.var, model.var)
    assert np.array_equal(clf.model_.n_states, [5, 4, 6])
    assert (np.diff(totals.sum(axis=1)) <= 0).all()  # Viterbi training does not increase the total cost
    first = {k: getattr(clf.model_, k).copy() for k in ("mean", "var", "stay", "adv")}, clf.totals_.copy()
    clf.fit(seqs, y)  # a second fit on the same object: the same bits
    for k, v in first[0].items():
        same_bits(getattr(clf.model_, k), v)
    same_bits(clf.totals_, first[1])
    queries, yq = word_sequences(141)
    q, nq = pad([(s - mean) / std for s in queries])
    ws, wl = H.score(model, q, nq)
    same_bits(clf.score_samples(queries), ws)
    pred = clf.predict(queries)
    assert np.array_equal(pred, classes[wl]) and np.mean(pred == yq) > 0.9
    assert clf.evaluate(queries, yq)["accuracy"] == float(np.mean(classes[wl] == yq))
    # the device surface under it
    score, label = hmm_score(clf.model_, q, nq, with_labels=True)
    same_bits(score.cpu().numpy(), ws)
    assert np.array_equal(label.cpu().numpy(), wl)
    assign = np.where(np.arange(len(y)) % 5 == 0, -1, codes)
    score, seg, start, members = hmm_align(clf.model_, X, n, assign=assign)
    start, members = start.cpu().numpy(), members.cpu().numpy()
    wa, wg = H.align(model, X, n, start, members)
    same_bits(score.cpu().numpy(), wa)
    assert np.array_equal(seg.cpu().numpy(), wg) and len(members) == int((assign >= 0).sum())
    only = hmm_align(clf.model_, X, n, groups=(start, members), with_seg=False)
    assert only[1] is None
    same_bits(only[0].cpu().numpy(), wa)
    # a class whose members are all shorter than its model
    with pytest.raises(ValueError):
        create_classifier('hmm', n_states=[5, 32, 5], n_iter=1).fit([s[:20] for s in seqs], y)
    # shorter members are left out of the statistics, the others train the model
    short = [s[:3] if i in (0, 3) else s for i, s in enumerate(seqs)]
    clf2 = create_classifier('hmm', n_states=5, n_iter=2).fit(short, y)
    frames = np.concatenate(short)
    X2, n2 = pad([(s - frames.mean(axis=0)) / frames.std(axis=0) for s in short])
    model2, totals2 = H.fit(X2, n2, codes, 5, n_iter=2)
    same_bits(clf2.model_.mean, model2.mu)
    same_bits(clf2.totals_, totals2)


def test_align_and_accumulate_in_a_graph():
    """dsp_hmm_align followed by dsp_hmm_accumulate (no allocation, no sync, the counts zeroed by a
    kernel) captured in a single-stream graph and replayed twice: the eager calls' bits."""
    import torch
    from src import _hip
    lib = _hip.lib()
    model, x, n, _ = table_case(2)
    x = np.nan_to_num(x)
    start, members = csr(table_groups(np.random.default_rng(150), len(x)))
    ws_, wg = H.align(model, x, n, start, members)
    want = H.accumulate(model.mu, model.var, STATES, x, n, start, members, wg, ws_, 1e-3)
    (N, T, F), (C, Smax), P = x.shape, model.mu.shape[:2], len(members)
    keep, margs = _model_args(model)
    t = [_dev(x, torch.float64), _dev(n, torch.int32), _dev(start, torch.int32), _dev(members, torch.int32),
         _dev(model.mu, torch.float64), _dev(model.var, torch.float64), _dev(np.asarray(STATES, np.int32), torch.int32)]
    score = torch.empty(P, dtype=torch.float64, device="cuda")
    seg = torch.empty((P, Smax), dtype=torch.int32, device="cuda")
    out = [torch.empty((C, Smax, F), dtype=torch.float64, device="cuda"), torch.empty((C, Smax, F), dtype=torch.float64, device="cuda"),
           torch.empty((C, Smax), dtype=torch.int32, device="cuda"), torch.empty(C, dtype=torch.int32, device="cuda"),
           torch.empty(C, dtype=torch.float64, device="cuda")]
    ws, nbytes = _workspace(C, N, P, T, F, Smax)

    def call():
        rc = lib.dsp_hmm_align(*margs, _hip.ptr(t[0]), _hip.ptr(t[1]), N, T, F, _hip.ptr(t[2]), _hip.ptr(t[3]), P,
                               _hip.ptr(score), _hip.ptr(seg), _hip.ptr(ws), nbytes, _hip.stream_handle())
        assert rc == 0
        rc = lib.dsp_hmm_accumulate(_hip.ptr(t[4]), _hip.ptr(t[5]), _hip.ptr(t[6]), C, Smax, _hip.ptr(t[0]), _hip.ptr(t[1]), N,
                                    T, F, _hip.ptr(t[2]), _hip.ptr(t[3]), P, _hip.ptr(seg), _hip.ptr(score), 1e-3,
                                    *[_hip.ptr(o) for o in out], _hip.ptr(ws), nbytes, _hip.stream_handle())
        assert rc == 0

    call()
    torch.cuda.synchronize()
    check_accumulate([o.cpu().numpy() for o in out], want)
    assert np.array_equal(seg.cpu().numpy(), wg)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        for o in out + [score, seg]:
            o.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        check_accumulate([o.cpu().numpy() for o in out], want)
        same_bits(score.cpu().numpy(), ws_)
        assert np.array_equal(seg.cpu().numpy(), wg)


def _write_wav(path, data, width=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(width)
        w.setframerate(44100)
        w.writeframes(np.ascontiguousarray(data).tobytes())


def test_compare_with_hmm(tmp_path):
    """compare(dtw=True, hmm=True): the rows of compare(dtw=True) unchanged, plus 'HMM' whose sequence
    accuracy is the restatement's on the same split (3 words x 5 synthetic clips)."""
    import compare_feature_methods as cfm
    from sklearn.model_selection import train_test_split
    from src.synth import make_clip
    for c in range(3):
        d = tmp_path / ("w%d" % c)
        d.mkdir()
        for j in range(5):
            _write_wav(d / ("s%d.wav" % j), make_clip(3000 + 10 * c + j, n_samples=36000 + 1013 * j, label=c, n_classes=3))
    base = cfm.compare(str(tmp_path), dtw=True)
    res = cfm.compare(str(tmp_path), dtw=True, hmm=True)
    assert list(base) == ["KNN", "SVM", "Decision Tree", "KNN-DTW"] and list(res) == list(base) + ["HMM"]
    assert {k: res[k] for k in base} == base
    row = res["HMM"]
    assert row["statistical"] == res["KNN"]["statistical"] and row["diff"] == row["sequence"] - row["statistical"]
    _, X_seq, y, lengths = cfm.load_both_methods(str(tmp_path))
    lengths = np.asarray(lengths)
    tr, te = train_test_split(np.arange(len(y)), test_size=0.2, random_state=42, stratify=y)
    frames = np.concatenate([X_seq[i, :lengths[i]] for i in tr])
    mean, std = frames.mean(axis=0), frames.std(axis=0)
    std = np.where(std == 0, 1.0, std)
    a, la = pad([(X_seq[i, :lengths[i]] - mean) / std for i in te])
    b, lb = pad([(X_seq[i, :lengths[i]] - mean) / std for i in tr])
    classes, codes = np.unique(y[tr], return_inverse=True)
    model, _ = H.fit(b, lb, codes, 5, n_iter=10)
    _, label = H.score(model, a, la)
    assert row["sequence"] == float(np.mean(classes[label] == y[te]))
