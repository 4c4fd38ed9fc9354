"""GPU tests of csrc/dhmm_fb.hip (dsp_dhmm_forward, dsp_dhmm_expect) through the bare C ABI, and of the Python
surface on it.  Everything is compared with the numpy restatement of tests/dhmm_fb_reference.py on the raw
bits and the raw integers: there is no tolerance and no pair is left out.  Behind each sequence's length the
symbol rows hold garbage (-1, K, 2^31 - 1 and INT_MIN); NaN stands behind every model array, in the rows
behind each model's states and in padv[c, S-1]."""
import functools

import numpy as np
import pytest

import dhmm_fb_reference as R
import dhmm_reference as D
from device_outputs import Guarded, _dev, bits, csr

pytestmark = pytest.mark.gpu

STATES = [1, 2, 3, 31, 32, 5, 32, 1, 7, 2, 31]  # C = 11, mixed within one model set, Smax = 32
EDGE = [1, 2, 3, 4, 5, 6, 7, 8, 30, 31, 32, 33, 63, 64, 65, 1]  # 1, 2, S-1, S, S+1 of every model and 63 .. 65


def _nan_after(x):
    import torch
    return _dev(np.concatenate([np.asarray(x, np.float64).reshape(-1), np.full(64, np.nan)]), torch.float64)


def _int_after(x, fill=1 << 20):
    import torch
    return _dev(np.concatenate([np.asarray(x, np.int32).reshape(-1), np.full(64, fill, np.int32)]), torch.int32)


def _model_args(model):
    from src import _hip
    C, Smax, K = model.pemit.shape
    pe, ps, pa = model.pemit.copy(), model.pstay.copy(), model.padv.copy()
    for c, S in enumerate(model.n_states):
        if 1 <= S <= Smax:  # what is never read
            pe[c, S:], ps[c, S:], pa[c, S - 1:] = np.nan, np.nan, np.nan
    keep = [_nan_after(a) for a in (pe, ps, pa)] + [_int_after(model.n_states)]
    return keep, [_hip.ptr(t) for t in keep] + [C, Smax, K]


def _workspace(C, N, P, T, Smax, K):
    import torch
    from src import _hip
    nbytes = _hip.lib().dsp_dhmm_fb_workspace_bytes(C, N, P, T, Smax, K)
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes


def forward_raw(model, sym, n, want=(True, True, True)):
    """dsp_dhmm_forward through the bare C ABI -> [mant, expo, label], None where not asked for."""
    import torch
    from src import _hip
    N, T = sym.shape
    keep, margs = _model_args(model)
    C, Smax, K = margs[-3:]
    ts, tn = _int_after(sym, -5), _dev(np.asarray(n, np.int32), torch.int32)
    outs = [Guarded((N, C), torch.float64, -7.0), Guarded((N, C), torch.int32, -9), Guarded((N,), torch.int32, -9)]
    ws, nbytes = _workspace(C, N, 0, T, Smax, K)
    rc = _hip.lib().dsp_dhmm_forward(*margs, _hip.ptr(ts), _hip.ptr(tn), N, T,
                                     *[_hip.ptr(o.view) if w else None for o, w in zip(outs, want)], _hip.ptr(ws), nbytes,
                                     _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    got = [o.get() for o in outs]
    for i, w in enumerate(want):
        if not w:
            assert (got[i] == outs[i].fill).all()
            got[i] = None
    return got


def expect_raw(model, sym, n, start, members, want=(True, True, True)):
    """dsp_dhmm_expect through the bare C ABI -> [mant, expo, gamma, occ_emit, n_valid], None where not asked for."""
    import torch
    from src import _hip
    N, T = sym.shape
    keep, margs = _model_args(model)
    C, Smax, K = margs[-3:]
    P = len(members)
    ts, tn = _int_after(sym, -5), _dev(np.asarray(n, np.int32), torch.int32)
    tg, tm = _dev(np.asarray(start, np.int32), torch.int32), _int_after(members)
    outs = [Guarded((P,), torch.float64, -7.0), Guarded((P,), torch.int32, -9),
            Guarded((P, T, Smax) if want[2] else (1,), torch.float64, -7.0), Guarded((C, Smax, K), torch.float64, -7.0),
            Guarded((C,), torch.int32, -9)]
    want = tuple(want) + (True, True)
    ws, nbytes = _workspace(C, N, P, T, Smax, K)
    rc = _hip.lib().dsp_dhmm_expect(*margs, _hip.ptr(ts), _hip.ptr(tn), N, T, _hip.ptr(tg), _hip.ptr(tm), P,
                                    *[_hip.ptr(o.view) if w else None for o, w in zip(outs, want)], _hip.ptr(ws), nbytes,
                                    _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    got = [o.get() for o in outs]
    for i, w in enumerate(want):
        if not w:
            assert (got[i] == outs[i].fill).all()
            got[i] = None
    return got


NAMES = ("mant", "expo", "gamma", "occ_emit", "n_valid")


def check(got, want, names=NAMES):
    for g, w, name in zip(got, want, names):
        if g is None:
            continue
        assert g.shape == np.asarray(w).shape, (name, g.shape, np.asarray(w).shape)
        g, w = (bits(v) if np.asarray(v).dtype == np.float64 else np.asarray(v) for v in (g, w))
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


def check_forward(model, sym, n, want=None):
    want = want or R.forward(model, sym, n)
    check(forward_raw(model, sym, n), want, ("mant", "expo", "label"))
    return want


def check_expect(model, sym, n, start, members, want=None, with_gamma=True):
    want = want or R.expect(model, sym, n, start, members)
    check(expect_raw(model, sym, n, start, members, (True, True, with_gamma)), want)
    return want


@functools.lru_cache(maxsize=None)
def table_case(K, states=tuple(STATES), Smax=32):
    """Models of the given states against 130 symbol rows of T = 65 (two full tiles and a partial one)."""
    model = R.random_probs(list(states), Smax, K, seed=40 + K)
    n = D.random_symbols(130, 65, K, seed=50 + K)[1]
    n[:len(EDGE)] = EDGE
    n[66:66 + len(EDGE)] = EDGE  # the same lengths in lanes of the next wave
    sym, n = D.random_symbols(130, 65, K, seed=50 + K, lengths=n)
    return model, sym, n, R.forward(model, sym, n)


def table_groups(rng, N, C=11):
    """Groups of 1, 63, 64, 65, 130 and 0 members and more; sequence 7 under two models."""
    groups = [rng.integers(0, N, k).tolist() for k in (1, 63, 64, 65, 130, 0, 17, 40, 5, 70, 3)[:C]]
    groups[0] = [7]
    groups[-1].append(7)
    return groups


@pytest.mark.parametrize("K", (1, 2, 3, 64, 255, 256))
def test_tables(K):
    model, sym, n, want = table_case(K)
    mant = want[0]
    assert (mant == 0).any() and (mant > 0).sum() > 500
    check_forward(model, sym, n, want)
    start, members = csr(table_groups(np.random.default_rng(60 + K), len(sym)))
    we = check_expect(model, sym, n, start, members)
    owner = np.repeat(np.arange(11), np.diff(start))
    check((we[0], we[1]), (mant[members, owner], want[1][members, owner]))
    assert we[5].sum() > 100 and we[4][5] == 0 and np.array_equal(we[5], we[0] > 0)
    for p in np.flatnonzero(we[5])[::7]:  # the invariants of a posterior, from the reference's rows the device equals
        k = n[members[p]]
        assert np.abs(we[2][p, :k].sum(axis=1) - 1).max() < 1e-13 and not we[2][p, k:].any()


@pytest.mark.parametrize("states", ((3, 5, 2), (16, 9, 1), (8, 8), (17, 4)))
def test_smax_equal_to_the_largest_model(states):
    """Smax = 5, 16, 8 and 17: the 8-, 16- and 32-slot kernels, each with its last state in the last slot."""
    model, sym, n, want = table_case(64, states, max(states))
    assert (want[0] > 0).sum() > 100
    check_forward(model, sym, n, want)
    start, members = csr(table_groups(np.random.default_rng(61), len(sym), len(states)))
    we = check_expect(model, sym, n, start, members)
    assert we[2].shape[2] == max(states) and we[4].sum() >= 40


@pytest.mark.parametrize("N", (1, 63, 64, 65))
def test_partial_and_multiple_tiles(N):
    model, sym, n, want = table_case(64)
    check_forward(model, sym[:N], n[:N], tuple(w[:N] for w in want))
    start, members = csr([list(range(N)), [], list(range(N - 1, -1, -1))] + [[]] * 8)
    check_expect(model, sym[:N], n[:N], start, members)


def test_null_outputs():
    model, sym, n, want = table_case(64)
    for mask in range(8):
        sel = tuple(bool(mask >> i & 1) for i in range(3))
        check(forward_raw(model, sym, n, sel), want, ("mant", "expo", "label"))
    start, members = csr(table_groups(np.random.default_rng(62), len(sym)))
    we = R.expect(model, sym, n, start, members)
    for mask in range(8):
        check(expect_raw(model, sym, n, start, members, tuple(bool(mask >> i & 1) for i in range(3))), we)


def test_longest_sequences():
    """T = 1024 with 65 sequences (a full tile and a lane) at S = 32 (and S = 1), K = 64: lengths 1024, 1023, 1000,
    33, 32, 31, 1 and random ones."""
    model = R.random_probs([32, 1], 32, 64, seed=90)
    n = np.random.default_rng(92).integers(1, 1025, 65)
    n[:7] = [1024, 1023, 1000, 33, 32, 31, 1]
    sym, n = D.random_symbols(65, 1024, 64, seed=91, lengths=n)
    want = check_forward(model, sym, n)
    assert (want[0][[0, 1, 2, 3, 4], 0] > 0).all() and (want[0][[5, 6], 0] == 0).all() and (want[0][:, 1] > 0).all()
    assert want[1][0, 0] < -3000  # far below the smallest double as a plain probability
    start, members = csr([list(range(65)), list(range(64, -1, -1))])
    we = check_expect(model, sym, n, start, members)
    assert we[4].tolist() == [int((want[0][:, 0] > 0).sum()), 65]


def test_many_models():
    """C = 1030 models (two launches of at most 1024) against 321 rows (six tiles per model): 6180 tiles for 4096
    persistent waves, so a wave takes a second tile -- of another model, which it stages; K = 4, S <= 4."""
    rng = np.random.default_rng(100)
    C, N, T, K = 1030, 321, 8, 4
    model = R.random_probs(rng.integers(1, 5, C), 4, K, seed=101)
    sym, n = D.random_symbols(N, T, K, seed=102)
    check_forward(model, sym, n)
    start, members = csr([list(range(65))] * C)  # 1030 models x 65 sequences: two tiles per group
    check_expect(model, sym, n, start, members)


def _tiles(sizes):
    return sum((k + 63) // 64 for k in sizes)


def short_list_case(K, T, sizes, seed):
    """Models of 2, 1 and 17 states (Smax = 17: 32 slots) over rows of 1 .. 3 symbols reused through members."""
    model = R.random_probs([2, 1, 17], 17, K, seed=seed)
    sym, n = D.random_symbols(40, T, K, seed=seed + 1, lengths=np.random.default_rng(seed + 2).integers(1, 4, 40))
    rng = np.random.default_rng(seed + 3)
    members = rng.integers(0, 40, sum(sizes)).astype(np.int32)
    members[rng.choice(len(members), 20, replace=False)] = np.tile([-1, 40], 10)
    return model, sym, n, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), members


def test_pair_chunk_boundary():
    """K = 256 at 32 slots: a table G_p is 64 KiB, so the 256 MiB budget holds 4096 pairs.  4100 + 130 + 70 pairs:
    the first group's sum is carried across the chunk boundary, the second chunk starts inside it."""
    from src import _hip
    sizes = [4100, 130, 70]
    model, sym, n, start, members = short_list_case(256, 3, sizes, 170)
    # the crossing, from the library's own plan: the whole workspace is smaller than the list's tables (64 KiB
    # each), so they cannot all be held at once and the list is taken in more than one chunk
    nbytes = _hip.lib().dsp_dhmm_fb_workspace_bytes(3, 40, sum(sizes), 3, 17, 256)
    assert 0 < nbytes < sum(sizes) * 256 * 32 * 8
    we = check_expect(model, sym, n, start, members, with_gamma=False)
    assert 2000 < we[4][0] < 4100 and we[4][1] > 100 and we[4][2] == 0


def test_wave_area_cap():
    """T = 64 at 32 slots: a wave's A rows are 1 MiB, so the 256 MiB budget holds 256 waves.  20 000 + 200 + 64
    pairs are 318 tiles: some waves take a second tile and reuse their area."""
    from src import _hip
    sizes = [20000, 200, 64]
    model, sym, n, start, members = short_list_case(2, 64, sizes, 180)
    # the crossing, from the library's own plan: the whole workspace is smaller than one area (64 rows x 32 slots
    # x 64 lanes of doubles) per tile of the list, so some wave must take a second tile
    nbytes = _hip.lib().dsp_dhmm_fb_workspace_bytes(3, 40, sum(sizes), 64, 17, 2)
    assert 0 < nbytes < _tiles(sizes) * 64 * 32 * 512
    we = check_expect(model, sym, n, start, members, with_gamma=False)
    assert 8000 < we[4][0] < 20000 and we[4][1] > 150 and we[4][2] == 0


@pytest.mark.parametrize("corpus", ("same", "stride"))
def test_bank_conflict_extremes(corpus):
    """K = 256 at 32 slots.  "same": all 64 lanes of a tile carry the same symbol in every row (every read a
    broadcast).  "stride": lane i carries symbol (16 i + t) mod K: the 16 lanes of a read's lane group hit 16
    different rows of one bank window, the layout's worst conflict."""
    K, N, T = 256, 130, 40
    model = R.random_probs([32, 31, 7], 32, K, seed=110)
    lane, t = np.arange(N)[:, None], np.arange(T)[None, :]
    sym = ((37 * t + 5) % K + 0 * lane if corpus == "same" else (16 * lane + t) % K).astype(np.int32)
    n = np.random.default_rng(111).integers(30, T + 1, N).astype(np.int32)
    want = check_forward(model, sym, n)
    assert (want[0][n >= 32] > 0).all()
    start, members = csr([list(range(N))] * 3)
    check_expect(model, sym, n, start, members)


def test_zero_probabilities():
    """Zero emissions, an all-zero emission row (nothing passes that state), pstay = 0 (the state holds one
    frame) and padv = 0: zeros, never NaN."""
    model = R.random_probs([5, 5, 32, 4], 32, 8, seed=80)
    model.pemit[0, 1, [0, 3]], model.pemit[1, 2, :], model.pemit[2, 30, 5] = 0.0, 0.0, 0.0
    model.pstay[0, 2], model.padv[3, 1], model.pstay[2, 30] = 0.0, 0.0, 0.0
    sym, n = D.random_symbols(70, 40, 8, seed=81)
    want = check_forward(model, sym, n)
    assert (want[0][:, 1] == 0).all() and (want[0][:, 0] > 0).sum() > 10 and (want[0][n >= 2, 3] == 0).all()
    start, members = csr([list(range(70))] * 4)
    we = check_expect(model, sym, n, start, members)
    assert not np.isnan(we[2]).any() and we[4][1] == 0 and we[4][0] > 10
    check_forward(R.random_probs(STATES, 32, 8, seed=82, zeros=0.1), sym, n)


def test_deep_underflow():
    """tests/dhmm_fb_reference.py's underflow set: a subnormal, rounded cell; a likelihood that underflows to
    zero although a path exists.  In dsp_dhmm_expect rows 0 and 2 under models 0 and 2 end on that subnormal
    cell: their likelihood is non-zero, but D_{n-1} is the cell itself and 1 / D overflows, so the members are
    not valid and nothing of them reaches gamma, occ_emit or n_valid -- every output is finite."""
    model, sym, n = R.underflow_set()
    want = check_forward(model, sym, n)
    assert (want[1][0, [0, 2]] < -1022).all() and want[0][0, 1] == 0
    start, members = csr([[0, 1, 2]] * 3)
    we = check_expect(model, sym, n, start, members)
    assert we[5].tolist() == [False, True, False, False, True, False, False, True, False] and we[4].tolist() == [1, 1, 1]
    assert (we[0][[0, 2, 6, 8]] > 0).all() and np.isfinite(we[2]).all() and np.isfinite(we[3]).all() and not we[2][~we[5]].any()
    assert 0 < we[2][1, 2, 2] < 1e-150 and we[2][4, 2, 2] == 0  # the cell's posterior, and where it underflowed


def test_dyadic_corpus_and_label_ties():
    """Probabilities that are multiples of 1/8, n <= 8, S <= 4 (exact: the CPU test compares the restatement with
    a fractions.Fraction brute force); models 4 and 5 are copies of models 1 and 0: ties go to the smaller index."""
    model = R.dyadic_probs([4, 3, 2, 1, 3, 4], 4, 3, seed=3)
    for v in (model.pemit, model.pstay, model.padv):
        v[4], v[5] = v[1], v[0]
    sym, n = D.random_symbols(130, 8, 3, seed=4)
    mant, expo, label = check_forward(model, sym, n)
    assert not np.isin(label, [4, 5]).any() and len(set(label.tolist())) >= 3
    best = np.where(mant > 0, np.ldexp(mant, expo), -1.0)  # exact: the values are dyadic
    tied = (best == best.max(axis=1, keepdims=True)).sum(axis=1) > 1
    assert tied[label >= 0].sum() > 20 and np.array_equal(label[label >= 0], best.argmax(axis=1)[label >= 0])
    start, members = csr([list(range(130))] * 6)
    check_expect(model, sym, n, start, members)


def invalid_case():
    model, sym, n, _ = table_case(64)
    sym, n = sym.copy(), n.copy()
    n[[20, 21]] = [0, 66]
    for row, t, v in ((30, 0, 64), (31, n[31] // 2, -1), (32, n[32] - 1, 2 ** 31 - 1), (33, 5, -2 ** 31), (34, n[34] - 1, 64)):
        sym[row, t] = v
    states = np.array(STATES)
    states[[2, 9]] = [0, 33]
    return R.Prob(model.pemit, model.pstay, model.padv, states), sym, n


def test_invalid_input():
    """Lengths 0 and T + 1, n_states 0 and 33, members -1 and N and far outside, and one symbol outside [0, K) at
    the first, a middle and the last valid frame: zero likelihood, label -1 and a skipped member there, the
    restatement's values everywhere else."""
    bad, sym, n = invalid_case()
    assert n[31] > 4 and n[33] > 5
    mant, expo, label = check_forward(bad, sym, n)
    rows = [20, 21, 30, 31, 32, 33, 34]
    assert (mant[rows] == 0).all() and (mant[:, [2, 9]] == 0).all() and (label[rows] == -1).all() and (mant > 0).sum() > 500
    groups = table_groups(np.random.default_rng(70), len(sym))
    groups[3] += [-1, len(sym), 20, 21, 1 << 30, -(1 << 31), 30, 31, 32, 33, 34]
    groups[2] += [1, 2, 3]
    start, members = csr(groups)
    we = check_expect(bad, sym, n, start, members)
    assert not we[5][start[4] - 11:start[4]].any() and we[4][2] == 0 and we[4][9] == 0 and we[4][3] > 10
    assert not we[2][~we[5]].any() and not we[3][[2, 9]].any()


def test_empty_list_and_empty_group():
    model, sym, n, _ = table_case(64)
    got = expect_raw(model, sym, n, np.zeros(12, np.int32), np.zeros(0, np.int32))
    assert got[0].shape == (0,) and got[2].shape == (0, 65, 32) and not got[3].any() and not got[4].any()
    start, members = csr([[], [3, 4]] + [[]] * 8 + [[5]])
    we = check_expect(model, sym, n, start, members)
    assert we[4].tolist() == [0, int(we[5][0]) + int(we[5][1])] + [0] * 8 + [int(we[5][2])]


def test_list_order():
    """occ_emit adds the members' tables in list order: reversing the first group changes the bits, in the
    restatement and on the device alike; n_valid and the pairs' own results only move with their pairs."""
    model, sym, n, _ = table_case(3)
    start, members = csr([[]] * 5 + [list(range(5, 45))] + [[]] * 4 + [list(range(130))])  # models of 5 and 31 states
    we = check_expect(model, sym, n, start, members)
    perm = np.r_[39:-1:-1, 40:len(members)]
    other = R.expect(model, sym, n, start, members[perm])
    assert not np.array_equal(bits(other[3][5]), bits(we[3][5])) and np.array_equal(bits(other[3][10]), bits(we[3][10]))
    assert np.array_equal(other[4], we[4]) and np.array_equal(bits(other[0]), bits(we[0][perm]))
    check_expect(model, sym, n, start, members[perm], other)


def test_forward_and_expect_in_a_graph():
    """dsp_dhmm_forward followed by dsp_dhmm_expect (no allocation, no sync, every output zeroed by a kernel)
    captured in a single-stream graph and replayed twice: the eager calls' bits."""
    import torch
    from src import _hip
    lib = _hip.lib()
    model, sym, n, wf = table_case(64)
    start, members = csr(table_groups(np.random.default_rng(150), len(sym)))
    we = R.expect(model, sym, n, start, members)
    (N, T), (C, Smax, K), P = sym.shape, model.pemit.shape, len(members)
    keep, margs = _model_args(model)
    t = [_dev(sym, torch.int32), _dev(n, torch.int32), _dev(start, torch.int32), _dev(members, torch.int32)]
    f64, i32 = torch.float64, torch.int32
    fo = [torch.empty((N, C), dtype=f64, device="cuda"), torch.empty((N, C), dtype=i32, device="cuda"),
          torch.empty(N, dtype=i32, device="cuda")]
    eo = [torch.empty(P, dtype=f64, device="cuda"), torch.empty(P, dtype=i32, device="cuda"),
          torch.empty((P, T, Smax), dtype=f64, device="cuda"), torch.empty((C, Smax, K), dtype=f64, device="cuda"),
          torch.empty(C, dtype=i32, device="cuda")]
    ws, nbytes = _workspace(C, N, P, T, Smax, K)

    def call():
        rc = lib.dsp_dhmm_forward(*margs, _hip.ptr(t[0]), _hip.ptr(t[1]), N, T, *[_hip.ptr(o) for o in fo], _hip.ptr(ws),
                                  nbytes, _hip.stream_handle())
        assert rc == 0
        rc = lib.dsp_dhmm_expect(*margs, _hip.ptr(t[0]), _hip.ptr(t[1]), N, T, _hip.ptr(t[2]), _hip.ptr(t[3]), P,
                                 *[_hip.ptr(o) for o in eo], _hip.ptr(ws), nbytes, _hip.stream_handle())
        assert rc == 0

    def verify():
        torch.cuda.synchronize()
        check([o.cpu().numpy() for o in fo], wf, ("mant", "expo", "label"))
        check([o.cpu().numpy() for o in eo], we)

    call()
    verify()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        for o in fo + eo:
            o.fill_(-5)
        g.replay()
        verify()


def test_python_surface():
    """dhmm_forward, DhmmUpdater.expect and dhmm_posterior against the restatement."""
    from src.pipeline import DhmmProbSet, DhmmUpdater, dhmm_forward, dhmm_nll, dhmm_posterior
    model, sym, n, wf = table_case(64, (3, 5, 2), 5)
    prob = DhmmProbSet.from_arrays(model.pemit, model.pstay, model.padv, model.n_states)
    mant, expo = dhmm_forward(prob, sym, n)
    check((mant.cpu().numpy(), expo.cpu().numpy()), wf)
    out = dhmm_forward(prob, sym, n, with_labels=True)
    assert len(out) == 3 and out[2].is_cuda
    check([o.cpu().numpy() for o in out], wf, ("mant", "expo", "label"))
    check((dhmm_nll(mant, expo),), (R.nll(wf[0], wf[1]),), ("nll",))
    start, members = csr(table_groups(np.random.default_rng(63), len(sym), 3))
    we = R.expect(model, sym, n, start, members)
    up = DhmmUpdater(sym, n, start, members)
    for _ in range(2):  # the updater's workspace is reused
        got = up.expect(prob, with_gamma=True)
        check([got[i].cpu().numpy() for i in (0, 1, 4, 2, 3)], we)
    assert len(up.expect(prob)) == 4
    assign = np.where(np.arange(len(n)) % 5 == 0, -1, np.arange(len(n)) % 3)
    gamma, gs, gm = dhmm_posterior(prob, sym, n, assign=assign)
    wa = R.expect(model, sym, n, gs.cpu().numpy(), gm.cpu().numpy())
    check((gamma.cpu().numpy(),), (wa[2],), ("gamma",))
    gamma, _, _ = dhmm_posterior(prob, sym, n, groups=(start, members))
    check((gamma.cpu().numpy(),), (we[2],), ("gamma",))


def word_sequences(seed, per_class=66):
    """3 classes x 66 sequences of 6 .. 14 frames, F = 2, drawn from known left-to-right models; the classes
    interleaved, labels 2, 7, 12."""
    rng = np.random.default_rng(seed)
    means = np.random.default_rng(7).normal(0, 2.0, (3, 3, 2)) * [1.0, 40.0]
    seqs, y = [], []
    for i in range(3 * per_class):
        c, k = i % 3, int(rng.integers(6, 15))
        cuts = np.sort(rng.choice(np.arange(1, k), 2, replace=False))
        state = np.searchsorted(cuts, np.arange(k), side="right")
        seqs.append(means[c, state] + rng.normal(0, 1.2, (k, 2)) * [1.0, 40.0])
        y.append(5 * c + 2)
    return seqs, np.array(y)


def pad(seqs):
    n = np.array([len(s) for s in seqs], np.int32)
    out = np.zeros((len(seqs), int(n.max()), seqs[0].shape[1]))
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out, n


def test_baum_welch_classifier():
    """DiscreteHmmClassifier(training='baum_welch', scoring='forward') against the restatement's whole fit and
    predict on 198 short sequences; decode on it equals dhmm_decode on prob_.to_costs(); the Viterbi-trained
    classifier with scoring='forward' scores with the set built from its last counts."""
    from src.models import create_classifier
    from src.pipeline import DhmmProbSet, dhmm_decode
    seqs, y = word_sequences(140)
    queries, yq = word_sequences(141, per_class=20)
    frames = np.concatenate(seqs)
    mean, std = frames.mean(axis=0), frames.std(axis=0)
    X, n = pad([(s - mean) / std for s in seqs])
    q, nq = pad([(s - mean) / std for s in queries])
    clf = create_classifier('dhmm', n_states=3, n_codes=8, n_iter=3, training='baum_welch', scoring='forward').fit(seqs, y)
    classes, codes = np.unique(y, return_inverse=True)
    cb, prob, totals = R.fit(X, n, codes, 3, 8, n_iter=3)
    assert clf.n_iter_ == 3 and clf.totals_.shape == (3, 3)
    check((clf.tokenizer_.codebook_, clf.totals_, clf.prob_.pemit, clf.prob_.pstay, clf.prob_.padv),
          (cb, totals, prob.pemit, prob.pstay, prob.padv), ("codebook", "totals", "pemit", "pstay", "padv"))
    assert (np.diff(totals.sum(axis=1)) < 0).all()  # each round lowers the total negative log-likelihood
    costs = R.to_costs(prob)
    check((clf.model_.emit, clf.model_.stay, clf.model_.adv), (costs.emit, costs.stay, costs.adv), ("emit", "stay", "adv"))
    sym = D.tokenize(cb, q, nq)
    mant, expo, label = R.forward(prob, sym, nq)
    check((clf.score_samples(queries),), (R.nll(mant, expo),), ("nll",))
    pred = clf.predict(queries)
    assert np.array_equal(pred, classes[label]) and np.mean(pred == yq) > 0.8
    assert clf.evaluate(queries, yq)["accuracy"] == float(np.mean(classes[label] == yq))
    with pytest.raises(ValueError):
        clf.predict([q[0, :2]])
    # connected words: always the cost form of the same models
    utter = [np.concatenate([queries[0], queries[1]]), queries[2]]
    words, starts = clf.decode(utter)
    U, nu = pad([(u - mean) / std for u in utter])
    _, n_words, w, s0, _ = dhmm_decode(DhmmProbSet.from_arrays(prob.pemit, prob.pstay, prob.padv, prob.n_states).to_costs(),
                                       D.tokenize(cb, U, nu), nu)
    n_words, w, s0 = (v.cpu().numpy() for v in (n_words, w, s0))
    for i in range(2):
        assert np.array_equal(words[i], classes[w[i, :n_words[i]]]) and np.array_equal(starts[i], s0[i, :n_words[i]])
    assert len(words[0]) >= 2
    # Viterbi training, forward scoring
    vit = create_classifier('dhmm', n_states=3, n_codes=8, n_iter=3, scoring='forward').fit(seqs, y)
    base = create_classifier('dhmm', n_states=3, n_codes=8, n_iter=3).fit(seqs, y)
    check((vit.model_.emit, vit.totals_), (base.model_.emit, base.totals_), ("emit", "totals"))
    # prob_ holds the last round's counts in DhmmProbSet's form: the same models as model_, up to the logarithm
    assert np.allclose(np.exp(-vit.model_.emit), vit.prob_.pemit, rtol=1e-14) and np.allclose(np.exp(-vit.model_.stay), vit.prob_.pstay, rtol=1e-14)
    mant, expo, label = R.forward(R.Prob(vit.prob_.pemit, vit.prob_.pstay, vit.prob_.padv, [3, 3, 3]), sym, nq)
    check((vit.score_samples(queries),), (R.nll(mant, expo),), ("nll",))
    assert np.array_equal(vit.predict(queries), classes[label])


def _write_wav(path, data):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(np.ascontiguousarray(data).tobytes())


def test_compare_with_dhmm_bw(tmp_path):
    """compare(dhmm=True, dhmm_bw=True): the rows of compare(dhmm=True) unchanged, plus 'VQ-HMM (BW)' after
    'VQ-HMM' whose sequence accuracy is the restatement's on the same split (3 words x 5 synthetic clips)."""
    import compare_feature_methods as cfm
    from sklearn.model_selection import train_test_split
    from src.synth import make_clip
    for c in range(3):
        d = tmp_path / ("w%d" % c)
        d.mkdir()
        for j in range(5):
            _write_wav(d / ("s%d.wav" % j), make_clip(3000 + 10 * c + j, n_samples=36000 + 1013 * j, label=c, n_classes=3))
    base = cfm.compare(str(tmp_path), dhmm=True)
    res = cfm.compare(str(tmp_path), dhmm=True, dhmm_bw=True)
    assert list(base)[-1] == "VQ-HMM" and list(res) == list(base) + ["VQ-HMM (BW)"]
    assert {k: res[k] for k in base} == base
    row = res["VQ-HMM (BW)"]
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
    cb, prob, _ = R.fit(b, lb, codes, 5, 64)
    label = R.forward(prob, D.tokenize(cb, a, la), la)[2]
    assert row["sequence"] == float(np.mean(classes[label] == y[te]))
