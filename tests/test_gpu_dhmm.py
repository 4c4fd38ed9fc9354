"""GPU tests of csrc/dhmm.hip (dsp_dhmm_score, dsp_dhmm_align, dsp_dhmm_accumulate) through the bare C ABI,
and of the Python surface on it.  Everything is compared with the numpy restatement of
tests/dhmm_reference.py on the raw bits and the raw integers: there is no tolerance and no pair is left
out.  Behind each sequence's length the symbol rows hold garbage: -1, K, 2^31 - 1 and INT_MIN."""
import functools
import wave

import numpy as np
import pytest

import dhmm_reference as D
from device_outputs import Guarded, _dev, bits, csr

pytestmark = pytest.mark.gpu

STATES = [1, 2, 3, 31, 32, 5, 32, 1, 7, 2, 31]  # C = 11, mixed within one model set, Smax = 32


def _nan_after(x):
    """A float64 input followed by NaN: a read past its end would poison a result."""
    import torch
    return _dev(np.concatenate([np.asarray(x, np.float64).reshape(-1), np.full(64, np.nan)]), torch.float64)


def _int_after(x, fill=1 << 20):
    import torch
    return _dev(np.concatenate([np.asarray(x, np.int32).reshape(-1), np.full(64, fill, np.int32)]), torch.int32)


def _model_args(model):
    from src import _hip
    keep = [_nan_after(a) for a in (model.emit, model.stay, model.adv)] + [_int_after(model.n_states)]
    C, Smax, K = model.emit.shape
    return keep, [_hip.ptr(t) for t in keep] + [C, Smax, K]


def _workspace(C, N, P, T, Smax, K):
    import torch
    from src import _hip
    nbytes = _hip.lib().dsp_dhmm_workspace_bytes(C, N, P, T, Smax, K)
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes


def score_raw(model, sym, n, with_score=True, with_label=True):
    """dsp_dhmm_score through the bare C ABI -> (score, label), None where not asked for."""
    import torch
    from src import _hip
    N, T = sym.shape
    keep, margs = _model_args(model)
    C, Smax, K = margs[-3:]
    ts, tn = _int_after(sym, -5), _dev(np.asarray(n, np.int32), torch.int32)
    gs, gl = Guarded((N, C), torch.float64, -7.0), Guarded((N,), torch.int32, -9)
    ws, nbytes = _workspace(C, N, 0, T, Smax, K)
    rc = _hip.lib().dsp_dhmm_score(*margs, _hip.ptr(ts), _hip.ptr(tn), N, T, _hip.ptr(gs.view) if with_score else None,
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


def align_raw(model, sym, n, start, members, with_score=True, with_seg=True):
    """dsp_dhmm_align through the bare C ABI -> (score, seg), None where not asked for."""
    import torch
    from src import _hip
    N, T = sym.shape
    keep, margs = _model_args(model)
    C, Smax, K = margs[-3:]
    P = len(members)
    ts, tn = _int_after(sym, -5), _dev(np.asarray(n, np.int32), torch.int32)
    tg, tm = _dev(np.asarray(start, np.int32), torch.int32), _int_after(members)
    gs, gg = Guarded((P,), torch.float64, -7.0), Guarded((P, Smax), torch.int32, -9)
    ws, nbytes = _workspace(C, N, P, T, Smax, K)
    rc = _hip.lib().dsp_dhmm_align(*margs, _hip.ptr(ts), _hip.ptr(tn), N, T, _hip.ptr(tg), _hip.ptr(tm), P,
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


def accumulate_raw(n_states, K, sym, n, start, members, seg, score):
    """dsp_dhmm_accumulate through the bare C ABI -> (cnt_emit, cnt, n_valid, total)."""
    import torch
    from src import _hip
    N, T = sym.shape
    C, Smax, P = len(n_states), np.asarray(seg).shape[1], len(members)
    tin = [_int_after(n_states), _int_after(sym, -5), _dev(np.asarray(n, np.int32), torch.int32),
           _dev(np.asarray(start, np.int32), torch.int32), _int_after(members), _int_after(seg), _nan_after(score)]
    out = [Guarded((C, Smax, K), torch.int32, -9), Guarded((C, Smax), torch.int32, -9), Guarded((C,), torch.int32, -9),
           Guarded((C,), torch.float64, -7.0)]
    ws, nbytes = _workspace(C, N, P, T, Smax, K)
    p = [_hip.ptr(t) for t in tin]
    rc = _hip.lib().dsp_dhmm_accumulate(p[0], C, Smax, K, p[1], p[2], N, T, p[3], p[4], P, p[5], p[6],
                                        *[_hip.ptr(o.view) for o in out], _hip.ptr(ws), nbytes, _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    return tuple(o.get() for o in out)


def same_bits(got, want):
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]


def check_accumulate(got, want):
    for g, w, name in zip(got, want, ("cnt_emit", "cnt", "n_valid", "total")):
        if g.dtype == np.float64:
            assert np.array_equal(bits(g), bits(w)), (name, np.argwhere(bits(g) != bits(w))[:5])
        else:
            assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


EDGE = [1, 2, 3, 4, 5, 6, 8, 30, 31, 32, 33, 63, 64, 65, 1]  # 1, 2, S-1, S, S+1 of every model and 63 .. 65


@functools.lru_cache(maxsize=None)
def table_case(K, states=tuple(STATES), Smax=32):
    """Models of the given states against 130 symbol rows of T = 65 (two full tiles and a partial one)."""
    model = D.random_models(list(states), Smax, K, seed=40 + K)
    sym, n = D.random_symbols(130, 65, K, seed=50 + K)
    n[:len(EDGE)] = EDGE
    n[66:66 + len(EDGE)] = EDGE  # the same lengths in lanes of the next wave
    sym, n = D.random_symbols(130, 65, K, seed=50 + K, lengths=n)
    return model, sym, n, D.score(model, sym, n)


def table_groups(rng, N, C=11):
    """Groups of 1, 63, 64, 65, 130 and 0 members and more; sequence 7 under two models."""
    groups = [rng.integers(0, N, k).tolist() for k in (1, 63, 64, 65, 130, 0, 17, 40, 5, 70, 3)[:C]]
    groups[0] = [7]
    groups[-1].append(7)
    return groups


@pytest.mark.parametrize("K", (1, 2, 3, 64, 255, 256))
def test_tables(K):
    model, sym, n, (ws, wl) = table_case(K)
    assert np.isinf(ws).any() and np.isfinite(ws).sum() > 500 and not np.isnan(ws).any()
    score, label = score_raw(model, sym, n)
    same_bits(score, ws)
    assert np.array_equal(label, wl)
    start, members = csr(table_groups(np.random.default_rng(60 + K), len(sym)))
    wa, wg = D.align(model, sym, n, start, members)
    owner = np.repeat(np.arange(11), np.diff(start))
    same_bits(wa, ws[members, owner])
    score, seg = align_raw(model, sym, n, start, members)
    same_bits(score, wa)
    assert np.array_equal(seg, wg), np.argwhere(seg != wg)[:5]
    for p in np.flatnonzero(np.isfinite(score)):  # the invariants, from the device's own output alone
        S = STATES[owner[p]]
        assert seg[p, 0] == 0 and (np.diff(seg[p, :S]) > 0).all() and seg[p, S - 1] < n[members[p]] and (seg[p, S:] == -1).all()
    assert (seg[np.isinf(score)] == -1).all()


@pytest.mark.parametrize("states", ((3, 5, 2), (16, 9, 1), (8, 8), (17, 4)))
def test_smax_equal_to_the_largest_model(states):
    """Smax = 5, 16, 8 and 17: the 8-, 16- and 32-slot kernels, each with its last state in the last slot."""
    model, sym, n, (ws, wl) = table_case(64, states, max(states))
    score, label = score_raw(model, sym, n)
    same_bits(score, ws)
    assert np.array_equal(label, wl) and np.isfinite(ws).sum() > 100
    start, members = csr(table_groups(np.random.default_rng(61), len(sym), len(states)))
    wa, wg = D.align(model, sym, n, start, members)
    score, seg = align_raw(model, sym, n, start, members)
    same_bits(score, wa)
    assert np.array_equal(seg, wg) and seg.shape[1] == max(states)


@pytest.mark.parametrize("N", (1, 63, 64, 65))
def test_partial_and_multiple_tiles(N):
    model, sym, n, (ws, wl) = table_case(64)
    score, label = score_raw(model, sym[:N], n[:N])
    same_bits(score, ws[:N])
    assert np.array_equal(label, wl[:N])


def test_null_outputs():
    model, sym, n, (ws, wl) = table_case(64)
    only_s, only_l = score_raw(model, sym, n, with_label=False), score_raw(model, sym, n, with_score=False)
    same_bits(only_s[0], ws)
    assert only_s[1] is None and only_l[0] is None and np.array_equal(only_l[1], wl)
    start, members = csr(table_groups(np.random.default_rng(62), len(sym)))
    wa, wg = D.align(model, sym, n, start, members)
    only_s = align_raw(model, sym, n, start, members, with_seg=False)
    only_g = align_raw(model, sym, n, start, members, with_score=False)
    same_bits(only_s[0], wa)
    assert only_s[1] is None and only_g[0] is None and np.array_equal(only_g[1], wg)
    assert align_raw(model, sym, n, start, members, with_score=False, with_seg=False) == (None, None)


def test_longest_sequences():
    """One tile at T = 1024 with S = 32 (and S = 1), K = 64: lengths 1024, 1000, 32, 31 and 1."""
    model = D.random_models([32, 1], 32, 64, seed=90)
    sym, n = D.random_symbols(5, 1024, 64, seed=91, lengths=[1024, 1000, 32, 31, 1])
    start, members = csr([[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]])
    ws, wg = D.align(model, sym, n, start, members)
    assert np.isfinite(ws[[0, 1, 2]]).all() and np.isinf(ws[[3, 4]]).all() and np.isfinite(ws[5:]).all()
    score, seg = align_raw(model, sym, n, start, members)
    same_bits(score, ws)
    assert np.array_equal(seg, wg) and seg[0, 31] > seg[0, 1] > 0
    same_bits(score_raw(model, sym, n)[0], np.stack([ws[:5], ws[5:][::-1]], axis=1))


def test_many_models():
    """C = 1030 models (two launches of at most 1024) against 321 rows (six tiles per model): 6180 tiles for
    4096 persistent waves, so a wave takes a second tile -- of another model, which it stages; K = 4, S <= 4."""
    rng = np.random.default_rng(100)
    C, N, T, K = 1030, 321, 8, 4
    model = D.random_models(rng.integers(1, 5, C), 4, K, seed=101)
    sym, n = D.random_symbols(N, T, K, seed=102)
    ws, wl = D.score(model, sym, n)
    score, label = score_raw(model, sym, n)
    same_bits(score, ws)
    assert np.array_equal(label, wl)
    start, members = csr([list(range(65))] * C)  # 1030 models x 65 sequences: two tiles per group
    wa, wg = D.align(model, sym, n, start, members)
    same_bits(wa, ws[:65].T.reshape(-1))
    score, seg = align_raw(model, sym, n, start, members)
    same_bits(score, wa)
    assert np.array_equal(seg, wg)


@pytest.mark.parametrize("corpus", ("same", "stride"))
def test_bank_conflict_extremes(corpus):
    """K = 256 at 32 slots.  "same": all 64 lanes of a tile carry the same symbol in every row (every read a
    broadcast).  "stride": lane i carries symbol (16 i + t) mod K -- with the pitch of 17 16-byte units,
    symbols that differ by a multiple of 16 start in the same bank window, so the 16 lanes of a read's lane
    group hit 16 different rows of one window, the layout's worst conflict."""
    K, N, T = 256, 130, 40
    model = D.random_models([32, 31, 7], 32, K, seed=110)
    lane, t = np.arange(N)[:, None], np.arange(T)[None, :]
    sym = ((37 * t + 5) % K + 0 * lane if corpus == "same" else (16 * lane + t) % K).astype(np.int32)
    n = np.random.default_rng(111).integers(30, T + 1, N).astype(np.int32)
    ws, wl = D.score(model, sym, n)
    assert np.isfinite(ws[n >= 32]).all()
    score, label = score_raw(model, sym, n)
    same_bits(score, ws)
    assert np.array_equal(label, wl)
    start, members = csr([list(range(N))] * 3)
    wa, wg = D.align(model, sym, n, start, members)
    score, seg = align_raw(model, sym, n, start, members)
    same_bits(score, wa)
    assert np.array_equal(seg, wg)


def test_tie_rule():
    """The dyadic corpus (costs that are multiples of 1/8) at N = 130, C = 11, K = 3: at least a tenth of the
    decided cells have a == b exactly, so the strict < decides the paths."""
    model = D.dyadic_models(STATES, 32, 3, seed=3)
    sym, n = D.random_symbols(130, 65, 3, seed=4)
    start, members = csr([list(range(130))] * 11)
    ties = [0, 0]
    ws, wg = D.align(model, sym, n, start, members, ties=ties)
    assert ties[0] > 50000 and ties[1] / ties[0] >= 0.10, ties
    score, seg = align_raw(model, sym, n, start, members)
    same_bits(score, ws)
    assert np.array_equal(seg, wg), np.argwhere(seg != wg)[:5]
    same_bits(score_raw(model, sym, n)[0], ws.reshape(11, 130).T)


def test_infinite_costs():
    """+inf emissions, an all-+inf emission row (nothing passes that state), stay = +inf (the state holds
    one frame) and adv = +inf: no NaN anywhere."""
    model = D.random_models([5, 5, 32, 4], 32, 8, seed=80)
    model.emit[0, 1, [0, 3]], model.emit[1, 2, :], model.emit[2, 30, 5] = np.inf, np.inf, np.inf
    model.stay[0, 2], model.adv[3, 1], model.stay[2, 30] = np.inf, np.inf, np.inf
    sym, n = D.random_symbols(70, 40, 8, seed=81)
    start, members = csr([list(range(70))] * 4)
    ws, wg = D.align(model, sym, n, start, members)
    assert not np.isnan(ws).any() and np.isinf(ws[70:140]).all() and np.isfinite(ws[:70]).sum() > 10
    assert np.isinf(ws[210:][n >= 2]).all()
    score, seg = align_raw(model, sym, n, start, members)
    same_bits(score, ws)
    assert np.array_equal(seg, wg)
    same_bits(score_raw(model, sym, n)[0], ws.reshape(4, 70).T)


def invalid_case():
    model, sym, n, _ = table_case(64)
    sym, n = sym.copy(), n.copy()
    n[[20, 21]] = [0, 66]
    for row, t, v in ((30, 0, 64), (31, n[31] // 2, -1), (32, n[32] - 1, 2 ** 31 - 1), (33, 5, -2 ** 31), (34, n[34] - 1, 64)):
        sym[row, t] = v
    states = np.array(STATES)
    states[[2, 9]] = [0, 33]
    return D.Model(model.emit, model.stay, model.adv, states), sym, n


def test_invalid_input():
    """Lengths 0 and T + 1, n_states 0 and 33, members -1 and N, and one symbol outside [0, K) at the first,
    a middle and the last valid frame: +inf and -1 there, the restatement's values everywhere else."""
    bad, sym, n = invalid_case()
    assert n[31] > 4 and n[33] > 5
    ws, wl = D.score(bad, sym, n)
    assert np.isinf(ws[[20, 21, 30, 31, 32, 33, 34]]).all() and np.isinf(ws[:, [2, 9]]).all() and np.isfinite(ws).sum() > 500
    score, label = score_raw(bad, sym, n)
    same_bits(score, ws)
    assert np.array_equal(label, wl) and (label[[20, 21, 30, 31, 32, 33, 34]] == -1).all()
    groups = table_groups(np.random.default_rng(70), len(sym))
    groups[3] += [-1, len(sym), 20, 21, 1 << 30, -(1 << 31), 30, 31, 32, 33, 34]
    start, members = csr(groups)
    wa, wg = D.align(bad, sym, n, start, members)
    assert np.isinf(wa[start[4] - 11:start[4]]).all() and np.isfinite(wa).sum() > 100
    score, seg = align_raw(bad, sym, n, start, members)
    same_bits(score, wa)
    assert np.array_equal(seg, wg) and (seg[np.isinf(score)] == -1).all()
    score, seg = align_raw(bad, sym, n, np.zeros(12, np.int32), np.zeros(0, np.int32))
    assert score.shape == (0,) and seg.shape == (0, 32)
    # in the re-estimation each of them is skipped whole
    lengths = np.where((members >= 0) & (members < len(sym)), n[np.clip(members, 0, len(sym) - 1)], 0)
    useg = D.uniform_seg(np.where((lengths >= 1) & (lengths <= 65), lengths, 0), np.clip(bad.n_states, 1, 32)[np.repeat(np.arange(11), np.diff(start))], 32)
    sc = np.random.default_rng(71).uniform(1, 9, len(members))
    want = D.accumulate(bad.n_states, 64, sym, n, start, members, useg, sc)
    assert want[2][2] == 0 and want[2][9] == 0 and 0 < want[2][3] <= 65 - 1
    check_accumulate(accumulate_raw(bad.n_states, 64, sym, n, start, members, useg, sc), want)


def accumulate_case(seed=120):
    """Five models (S = 4, 1, 6, 5, 3) over 90 rows of K = 7 symbols: groups of 40, 16, 17, 0 and 5 members in
    a shuffled order; model 3 has no member and model 4 only members that are skipped."""
    rng = np.random.default_rng(seed)
    N, T, K, S = 90, 30, 7, np.array([4, 1, 6, 5, 3])
    n = rng.integers(6, T + 1, N).astype(np.int32)
    n[80:] = 2
    sym, n = D.random_symbols(N, T, K, seed=seed + 1, lengths=n)
    groups = [rng.permutation(80)[:k].tolist() for k in (40, 16, 17, 0)] + [[80, 81, -1, N, 82]]
    start, members = csr(groups)
    owner = np.repeat(np.arange(5), np.diff(start))
    ok = (members >= 0) & (members < N)
    seg = D.uniform_seg(np.where(ok, n[np.where(ok, members, 0)], 0), S[owner], 6)
    return sym, n, K, S, start, members, seg, rng.uniform(1, 100, len(members))


def test_accumulate():
    sym, n, K, S, start, members, seg, score = accumulate_case()
    want = D.accumulate(S, K, sym, n, start, members, seg, score)
    assert want[2].tolist() == [40, 16, 17, 0, 0] and not want[0][3:].any() and want[3][3:].tolist() == [0.0, 0.0]
    assert want[1][1, 0] == n[members[40:56]].sum() and (want[0].sum(axis=2) == want[1]).all()
    check_accumulate(accumulate_raw(S, K, sym, n, start, members, seg, score), want)
    # permuting the list changes total's bits, in the restatement and on the device alike, and no count
    perm = np.r_[39:-1:-1, 40:len(members)]
    other = D.accumulate(S, K, sym, n, start, members[perm], seg[perm], score[perm])
    assert not np.array_equal(bits(other[3][0]), bits(want[3][0])) and np.array_equal(other[0], want[0])
    check_accumulate(accumulate_raw(S, K, sym, n, start, members[perm], seg[perm], score[perm]), other)
    # malformed seg rows are skipped: not starting at 0, not increasing, past the end, an n_states of 0
    seg2, S2 = seg.copy(), S.copy()
    seg2[0, 0], seg2[1, 2], seg2[2, 3], S2[1] = 1, seg2[1, 1], 1000, 0
    want2 = D.accumulate(S2, K, sym, n, start, members, seg2, score)
    assert want2[2].tolist() == [37, 0, 17, 0, 0]
    check_accumulate(accumulate_raw(S2, K, sym, n, start, members, seg2, score), want2)
    # P = 0: zeros everywhere
    got = accumulate_raw(S, K, sym, n, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros((0, 6), np.int32), np.zeros(0))
    assert not any(g.any() for g in got)


def test_accumulate_after_align():
    """dsp_dhmm_align's own seg and score as the input, K = 64 and S up to 32."""
    model, sym, n, _ = table_case(64)
    start, members = csr(table_groups(np.random.default_rng(130), len(sym)))
    score, seg = align_raw(model, sym, n, start, members)
    want = D.accumulate(STATES, 64, sym, n, start, members, seg, score)
    assert want[2][5] == 0 and want[2][4] > 20
    check_accumulate(accumulate_raw(STATES, 64, sym, n, start, members, seg, score), want)


def test_accumulate_long_list():
    """40 000 pairs over two models (S = 1, 2) and six rows of 1 .. 3 symbols reused through members (the
    call has no pair chunk; one launch covers the list): members -1 and N and the one-symbol rows under the
    two-state model are skipped; many atomic adds land on each count."""
    Smax, K, T, N = 32, 5, 3, 6
    sizes = [25000, 15000]
    P = sum(sizes)
    rng = np.random.default_rng(160)
    sym, n = D.random_symbols(N, T, K, seed=161, lengths=[3, 1, 2, 3, 2, 1])
    S = np.array([1, 2])
    members = rng.integers(0, N, P).astype(np.int32)
    members[rng.choice(P, 40, replace=False)] = np.tile([-1, N], 20)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    ok = (members >= 0) & (members < N)
    seg = D.uniform_seg(np.where(ok, n[np.where(ok, members, 0)], 0), S[np.repeat(np.arange(2), sizes)], Smax)
    score = rng.uniform(1, 100, P)
    want = D.accumulate(S, K, sym, n, start, members, seg, score)
    assert want[2][0] == int(ok[:sizes[0]].sum()) < sizes[0] and 5000 < want[2][1] < int(ok[sizes[0]:].sum())
    check_accumulate(accumulate_raw(S, K, sym, n, start, members, seg, score), want)


def test_align_and_accumulate_in_a_graph():
    """dsp_dhmm_align followed by dsp_dhmm_accumulate (no allocation, no sync, the counts zeroed by a kernel)
    captured in a single-stream graph and replayed twice: the eager calls' bits."""
    import torch
    from src import _hip
    lib = _hip.lib()
    model, sym, n, _ = table_case(64)
    start, members = csr(table_groups(np.random.default_rng(150), len(sym)))
    ws_, wg = D.align(model, sym, n, start, members)
    want = D.accumulate(STATES, 64, sym, n, start, members, wg, ws_)
    (N, T), (C, Smax, K), P = sym.shape, model.emit.shape, len(members)
    keep, margs = _model_args(model)
    t = [_dev(sym, torch.int32), _dev(n, torch.int32), _dev(start, torch.int32), _dev(members, torch.int32)]
    score = torch.empty(P, dtype=torch.float64, device="cuda")
    seg = torch.empty((P, Smax), dtype=torch.int32, device="cuda")
    out = [torch.empty((C, Smax, K), dtype=torch.int32, device="cuda"), torch.empty((C, Smax), dtype=torch.int32, device="cuda"),
           torch.empty(C, dtype=torch.int32, device="cuda"), torch.empty(C, dtype=torch.float64, device="cuda")]
    ws, nbytes = _workspace(C, N, P, T, Smax, K)

    def call():
        rc = lib.dsp_dhmm_align(*margs, _hip.ptr(t[0]), _hip.ptr(t[1]), N, T, _hip.ptr(t[2]), _hip.ptr(t[3]), P,
                                _hip.ptr(score), _hip.ptr(seg), _hip.ptr(ws), nbytes, _hip.stream_handle())
        assert rc == 0
        rc = lib.dsp_dhmm_accumulate(margs[3], C, Smax, K, _hip.ptr(t[0]), _hip.ptr(t[1]), N, T, _hip.ptr(t[2]), _hip.ptr(t[3]),
                                     P, _hip.ptr(seg), _hip.ptr(score), *[_hip.ptr(o) for o in out], _hip.ptr(ws), nbytes,
                                     _hip.stream_handle())
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


@functools.lru_cache(maxsize=None)
def scaled_words():
    seqs, y = word_sequences(140)
    frames = np.concatenate(seqs)
    mean, std = frames.mean(axis=0), frames.std(axis=0)
    X, n = pad([(s - mean) / std for s in seqs])
    queries, yq = word_sequences(141)
    q, nq = pad([(s - mean) / std for s in queries])
    return seqs, y, X, n, queries, yq, q, nq


def test_vq_tokenizer():
    from src.models import VqClassifier
    from src.pipeline import VqTokenizer
    _, _, X, n, _, _, q, nq = scaled_words()
    tok = VqTokenizer(16, n_iter=6, eps=0.02).fit(X, n)
    clf = VqClassifier(16, 6, 0.02, normalize=False).fit(X, np.zeros(len(X)), n)
    same_bits(tok.codebook_, clf.codebooks_[0])
    cb = D.tokenizer_fit(X, n, 16, 6, 0.02)
    same_bits(tok.codebook_, cb)
    sym = tok.transform(q, nq)
    assert sym.dtype.is_floating_point is False and sym.is_cuda and tuple(sym.shape) == q.shape[:2]
    want = D.tokenize(cb, q, nq)
    assert np.array_equal(sym.cpu().numpy(), want) and (want[np.arange(q.shape[1])[None, :] >= nq[:, None]] == -1).all()


@pytest.mark.parametrize("n_states,n_codes", ((1, 1), (3, 8), (5, 16)))
def test_discrete_hmm_classifier(n_states, n_codes):
    from src.models import create_classifier
    from src.pipeline import dhmm_align, dhmm_score
    seqs, y, X, n, queries, yq, q, nq = scaled_words()
    clf = create_classifier('dhmm', n_states=n_states, n_codes=n_codes, n_iter=6).fit(seqs, y)
    classes, codes = np.unique(y, return_inverse=True)
    cb, model, totals = D.fit(X, n, codes, n_states, n_codes, n_iter=6)
    assert 1 <= len(totals) <= 6 and clf.totals_.shape == totals.shape and clf.n_iter_ == len(totals)
    same_bits(clf.tokenizer_.codebook_, cb)
    same_bits(clf.totals_, totals)
    for name in ("emit", "stay", "adv"):
        same_bits(getattr(clf.model_, name), getattr(model, name))
    assert np.array_equal(clf.model_.n_states, [n_states] * 3)
    sym = D.tokenize(cb, q, nq)
    ws, wl = D.score(model, sym, nq)
    same_bits(clf.score_samples(queries), ws)
    pred = clf.predict(queries)
    assert np.array_equal(pred, classes[wl])
    assert clf.evaluate(queries, yq)["accuracy"] == float(np.mean(classes[wl] == yq))
    if n_codes > 1:
        assert np.mean(pred == yq) > 0.8
    # the device surface under it
    score, label = dhmm_score(clf.model_, sym, nq, with_labels=True)
    same_bits(score.cpu().numpy(), ws)
    assert np.array_equal(label.cpu().numpy(), wl)
    assign = np.where(np.arange(len(nq)) % 5 == 0, -1, codes)
    score, seg, start, members = dhmm_align(clf.model_, sym, nq, assign=assign)
    wa, wg = D.align(model, sym, nq, start.cpu().numpy(), members.cpu().numpy())
    same_bits(score.cpu().numpy(), wa)
    assert np.array_equal(seg.cpu().numpy(), wg)
    with pytest.raises(ValueError):
        clf.predict([q[0, :max(n_states - 1, 0)]] if n_states > 1 else [np.zeros((0, 2))])


def _write_wav(path, data, width=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(width)
        w.setframerate(44100)
        w.writeframes(np.ascontiguousarray(data).tobytes())


def test_compare_with_dhmm(tmp_path):
    """compare(vq=True, dhmm=True): the rows of compare(vq=True) unchanged, plus 'VQ-HMM' after 'VQ' whose
    sequence accuracy is the restatement's on the same split (3 words x 5 synthetic clips)."""
    import compare_feature_methods as cfm
    from sklearn.model_selection import train_test_split
    from src.synth import make_clip
    for c in range(3):
        d = tmp_path / ("w%d" % c)
        d.mkdir()
        for j in range(5):
            _write_wav(d / ("s%d.wav" % j), make_clip(3000 + 10 * c + j, n_samples=36000 + 1013 * j, label=c, n_classes=3))
    base = cfm.compare(str(tmp_path), vq=True)
    res = cfm.compare(str(tmp_path), vq=True, dhmm=True)
    assert list(base)[-1] == "VQ" and list(res) == list(base) + ["VQ-HMM"]
    assert {k: res[k] for k in base} == base
    row = res["VQ-HMM"]
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
    cb, model, _ = D.fit(b, lb, codes, 5, 64)
    _, label = D.score(model, D.tokenize(cb, a, la), la)
    assert row["sequence"] == float(np.mean(classes[label] == y[te]))
