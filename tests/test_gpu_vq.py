"""GPU tests of csrc/vq.hip (dsp_vq_score, dsp_vq_assign, dsp_vq_accumulate) through the bare C ABI, and
of the Python surface on it.  Everything is compared with the numpy restatement of tests/vq_reference.py
on the raw bits and the raw integers: distortions, codes and re-estimated codebooks are defined bit for
bit, so there is no tolerance and no pair is left out."""
import functools
import wave

import numpy as np
import pytest

import vq_reference as V
from device_outputs import Guarded, _dev, bits, csr

pytestmark = pytest.mark.gpu

CODES = [1, 2, 3, 16, 63, 64, 65, 255, 256, 7]  # C = 10, mixed within one codebook set


def _nan_after(x):
    """A float64 input followed by NaN: a read past its end would poison a result."""
    import torch
    return _dev(np.concatenate([np.asarray(x, np.float64).reshape(-1), np.full(64, np.nan)]), torch.float64)


def _int_after(x, n=64):
    """An int32 input followed by out-of-range values."""
    import torch
    return _dev(np.concatenate([np.asarray(x, np.int32).reshape(-1), np.full(n, 1 << 20, np.int32)]), torch.int32)


def _workspace(C, N, P, T, F, Kmax):
    import torch
    from src import _hip
    nbytes = _hip.lib().dsp_vq_workspace_bytes(C, N, P, T, F, Kmax)
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes


def score_raw(cb, n_codes, x, n, with_score=True, with_label=True):
    """dsp_vq_score through the bare C ABI -> (score, label), None where not asked for."""
    import torch
    from src import _hip
    (N, T, F), (C, Kmax) = x.shape, cb.shape[:2]
    tin = [_nan_after(cb), _int_after(n_codes), _nan_after(x), _dev(np.asarray(n, np.int32), torch.int32)]
    gs, gl = Guarded((N, C), torch.float64, -7.0), Guarded((N,), torch.int32, -9)
    ws, nbytes = _workspace(C, N, 0, T, F, Kmax)
    rc = _hip.lib().dsp_vq_score(_hip.ptr(tin[0]), _hip.ptr(tin[1]), C, Kmax, _hip.ptr(tin[2]), _hip.ptr(tin[3]), N, T, F,
                                 _hip.ptr(gs.view) if with_score else None, _hip.ptr(gl.view) if with_label else None,
                                 _hip.ptr(ws), nbytes, _hip.stream_handle())
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


def assign_raw(cb, n_codes, x, n, start, members, with_dist=True, with_code=True):
    """dsp_vq_assign through the bare C ABI -> (dist, code), None where not asked for."""
    import torch
    from src import _hip
    (N, T, F), (C, Kmax), P = x.shape, cb.shape[:2], len(members)
    tin = [_nan_after(cb), _int_after(n_codes), _nan_after(x), _dev(np.asarray(n, np.int32), torch.int32),
           _dev(np.asarray(start, np.int32), torch.int32), _int_after(members, 16)]
    gd, gc = Guarded((P,), torch.float64, -7.0), Guarded((P, T), torch.int32, -9)
    ws, nbytes = _workspace(C, N, P, T, F, Kmax)
    rc = _hip.lib().dsp_vq_assign(_hip.ptr(tin[0]), _hip.ptr(tin[1]), C, Kmax, _hip.ptr(tin[2]), _hip.ptr(tin[3]), N, T, F,
                                  _hip.ptr(tin[4]), _hip.ptr(tin[5]), P, _hip.ptr(gd.view) if with_dist else None,
                                  _hip.ptr(gc.view) if with_code else None, _hip.ptr(ws), nbytes, _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    dist, code = gd.get(), gc.get()
    if not with_dist:
        assert (dist == -7.0).all()
        dist = None
    if not with_code:
        assert (code == -9).all()
        code = None
    return dist, code


def accumulate_raw(cb_prev, n_codes, x, n, start, members, code, dist):
    """dsp_vq_accumulate through the bare C ABI -> (centroid, cnt, n_valid, total)."""
    import torch
    from src import _hip
    (N, T, F), (C, Kmax), P = x.shape, cb_prev.shape[:2], len(members)
    tin = [_nan_after(cb_prev), _int_after(n_codes), _nan_after(x), _dev(np.asarray(n, np.int32), torch.int32),
           _dev(np.asarray(start, np.int32), torch.int32), _int_after(members, 16), _int_after(code), _nan_after(dist)]
    out = [Guarded((C, Kmax, F), torch.float64, -7.0), Guarded((C, Kmax), torch.int32, -9), Guarded((C,), torch.int32, -9),
           Guarded((C,), torch.float64, -7.0)]
    ws, nbytes = _workspace(C, N, P, T, F, Kmax)
    p = [_hip.ptr(t) for t in tin]
    rc = _hip.lib().dsp_vq_accumulate(p[0], p[1], C, Kmax, p[2], p[3], N, T, F, p[4], p[5], P, p[6], p[7],
                                      *[_hip.ptr(o.view) for o in out], _hip.ptr(ws), nbytes, _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    return tuple(o.get() for o in out)


def same_bits(got, want):
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]


def check_accumulate(got, want):
    for g, w, name in zip(got, want, ("centroid", "cnt", "n_valid", "total")):
        if g.dtype == np.float64:
            assert np.array_equal(bits(g), bits(w)), (name, np.argwhere(bits(g) != bits(w))[:5])
        else:
            assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


def random_books(n_codes, Kmax, F, seed):
    """Codebooks [C, Kmax, F] of random reals, NaN behind each codebook's codewords (never read)."""
    cb = np.random.default_rng(seed).normal(0, 1, (len(n_codes), Kmax, F))
    cb[np.arange(Kmax)[None, :] >= np.asarray(n_codes)[:, None]] = np.nan
    return cb


def table_groups(rng, N, C=10):
    """Groups of 1, 63, 64, 65, 130 and 0 members and more; sequence 7 under two codebooks and twice under one."""
    groups = [rng.integers(0, N, k).tolist() for k in (1, 63, 64, 65, 130, 0, 17, 40, 5, 70)][:C]
    groups[0] = [7]
    groups[8] += [7, 7]
    return groups


@functools.lru_cache(maxsize=None)
def table_case(F, Kmax=256):
    """C = 10 codebooks of 1 .. 256 codewords against N = 130 sequences (two full tiles and a partial one)
    of T = 70: random reals, lengths covering 1, 2, 63, 64, 65 and T; NaN behind each sequence's frames and
    behind each codebook's codewords.  The reference is computed once and shared."""
    n_codes = np.minimum(np.array(CODES, np.int32), Kmax)
    cb = random_books(n_codes, Kmax, F, 40 + F)
    rng = np.random.default_rng(50 + F)
    N, T = 130, 70
    x, n = rng.normal(0, 1, (N, T, F)), rng.integers(1, T + 1, N).astype(np.int32)
    edge = [1, 2, 63, 64, 65, 70, 16, 17, 15, 32, 33, 1]
    n[:len(edge)] = edge
    n[64:64 + len(edge)] = edge  # the same lengths in lanes of the next tile
    n[128:] = [2, 65]
    x[np.arange(T)[None, :] >= n[:, None]] = np.nan
    want = V.score(np.nan_to_num(cb), n_codes, np.nan_to_num(x), n)
    start, members = csr(table_groups(np.random.default_rng(60 + F), N))
    wa = V.assign(np.nan_to_num(cb), n_codes, np.nan_to_num(x), n, start, members)
    return cb, n_codes, x, n, want, start, members, wa


@pytest.mark.parametrize("F", (1, 2, 3, 8))
def test_score_and_assign_table(F):
    cb, n_codes, x, n, (ws, wl), start, members, (wd, wc) = table_case(F)
    assert np.isfinite(ws).all() and len(set(wl.tolist())) > 1
    score, label = score_raw(cb, n_codes, x, n)
    same_bits(score, ws)
    assert np.array_equal(label, wl)
    owner = np.repeat(np.arange(10), np.diff(start))
    same_bits(wd, ws[members, owner])
    assert start[5] == start[6] and (members == 7).sum() >= 3
    dist, code = assign_raw(cb, n_codes, x, n, start, members)
    same_bits(dist, wd)
    assert np.array_equal(code, wc), np.argwhere(code != wc)[:5]
    # the invariants, from the device's own output alone
    assert ((code >= 0).sum(axis=1) == n[members]).all() and (code.max(axis=1) < n_codes[owner]).all()
    assert (code[np.arange(code.shape[1])[None, :] >= n[members][:, None]] == -1).all()


def test_kmax_equal_to_the_largest_codebook():
    """Kmax = 65 = the largest n_codes (the staged codebook is padded to 68 rows inside the kernel, not in memory)."""
    cb, n_codes, x, n, (ws, wl), start, members, (wd, wc) = table_case(2, 65)
    assert n_codes.max() == 65 and cb.shape[1] == 65
    score, label = score_raw(cb, n_codes, x, n)
    same_bits(score, ws)
    assert np.array_equal(label, wl)
    dist, code = assign_raw(cb, n_codes, x, n, start, members)
    same_bits(dist, wd)
    assert np.array_equal(code, wc)


def test_null_outputs():
    """Each of score / label / dist / code left NULL leaves its guard untouched; the other is unchanged."""
    cb, n_codes, x, n, (ws, wl), start, members, (wd, wc) = table_case(3)
    only_s = score_raw(cb, n_codes, x, n, with_label=False)
    only_l = score_raw(cb, n_codes, x, n, with_score=False)
    same_bits(only_s[0], ws)
    assert only_s[1] is None and only_l[0] is None and np.array_equal(only_l[1], wl)
    only_d = assign_raw(cb, n_codes, x, n, start, members, with_code=False)
    only_c = assign_raw(cb, n_codes, x, n, start, members, with_dist=False)
    same_bits(only_d[0], wd)
    assert only_d[1] is None and only_c[0] is None and np.array_equal(only_c[1], wc)


def test_longest_sequences():
    """One tile at T = 1024: lengths 1024, 1000 and 1."""
    n_codes = np.array([5, 1], np.int32)
    cb = random_books(n_codes, 8, 2, 90)
    rng = np.random.default_rng(91)
    x, n = rng.normal(0, 1, (3, 1024, 2)), np.array([1024, 1000, 1], np.int32)
    start, members = csr([[0, 1, 2], [2, 1, 0]])
    wd, wc = V.assign(np.nan_to_num(cb), n_codes, x, n, start, members)
    dist, code = assign_raw(cb, n_codes, x, n, start, members)
    same_bits(dist, wd)
    assert np.array_equal(code, wc) and (code[0] >= 0).all() and (code[1, 1000:] == -1).all() and (code[2, 1:] == -1).all()
    same_bits(score_raw(cb, n_codes, x, n)[0], np.stack([wd[:3], wd[3:][::-1]], axis=1))


def test_more_tiles_than_waves():
    """C = 1030 codebooks (two launches of at most 1024) against 321 sequences (six tiles per codebook):
    6144 tiles for 4096 persistent waves, so a wave takes a second tile; short sequences, K <= 4."""
    rng = np.random.default_rng(100)
    C, N, T, F = 1030, 321, 8, 2
    n_codes = rng.integers(1, 5, C).astype(np.int32)
    cb = random_books(n_codes, 4, F, 101)
    x, n = rng.normal(0, 1, (N, T, F)), rng.integers(1, T + 1, N).astype(np.int32)
    ws, wl = V.score(np.nan_to_num(cb), n_codes, x, n)
    score, label = score_raw(cb, n_codes, x, n)
    same_bits(score, ws)
    assert np.array_equal(label, wl)
    start, members = csr([list(range(N))] * C)
    wd, wc = V.assign(np.nan_to_num(cb), n_codes, x, n, start, members)
    same_bits(wd, ws.T.reshape(-1))
    dist, code = assign_raw(cb, n_codes, x, n, start, members)
    same_bits(dist, wd)
    assert np.array_equal(code, wc)


def test_tie_rule():
    """Integer frames and codewords uniform in [-3, 3], F = 2, K = 16, 130 sequences x 40 frames: at least
    a quarter of the frames have two or more codewords at the minimum, so the strict < decides their codes."""
    rng = np.random.default_rng(7)
    cb = rng.integers(-3, 4, (1, 16, 2)).astype(np.float64)
    x = rng.integers(-3, 4, (130, 40, 2)).astype(np.float64)
    n = np.full(130, 40, np.int32)
    d = ((x[:, :, None, :] - cb[0][None, None]) ** 2).sum(axis=3)
    frac = float(((d == d.min(axis=2, keepdims=True)).sum(axis=2) >= 2).mean())
    assert frac >= 0.25, frac
    start, members = csr([list(range(130))])
    wd, wc = V.assign(cb, [16], x, n, start, members)
    assert np.array_equal(wc, np.argmin(d, axis=2))
    dist, code = assign_raw(cb, [16], x, n, start, members)
    same_bits(dist, wd)
    assert np.array_equal(code, wc), np.argwhere(code != wc)[:5]
    same_bits(score_raw(cb, [16], x, n)[0][:, 0], wd)


def test_invalid_input():
    """Lengths 0 and T + 1, n_codes 0 and Kmax + 1, members -1 and N: +inf distances and all -1 codes there,
    the restatement's values everywhere else; label -1 on an all-+inf row; two identical codebooks tie to
    the smaller index; P = 0 writes nothing."""
    cb, n_codes, x, n, _, _, _, _ = table_case(2)
    x, n, n_codes, cb = x.copy(), n.copy(), n_codes.copy(), np.nan_to_num(cb)
    T, N = x.shape[1], len(x)
    n[[20, 21]] = [0, T + 1]
    n_codes[[2, 8]] = [0, 257]
    cb[5], n_codes[5] = cb[4], n_codes[4]  # codebooks 4 and 5 are identical
    ws, wl = V.score(cb, n_codes, np.nan_to_num(x), n)
    assert np.isinf(ws[[20, 21]]).all() and np.isinf(ws[:, [2, 8]]).all() and (wl[[20, 21]] == -1).all()
    score, label = score_raw(cb, n_codes, x, n)
    same_bits(score, ws)
    assert np.array_equal(label, wl) and (label != 5).all()
    same_bits(score[:, 4], score[:, 5])
    groups = table_groups(np.random.default_rng(70), N)
    groups[3] += [-1, N, 20, 21, 1 << 30, -(1 << 31)]
    start, members = csr(groups)
    wd, wc = V.assign(cb, n_codes, np.nan_to_num(x), n, start, members)
    assert np.isinf(wd).sum() >= 6 + len(groups[2]) + len(groups[8]) and np.isfinite(wd).sum() > 100
    dist, code = assign_raw(cb, n_codes, x, n, start, members)
    same_bits(dist, wd)
    assert np.array_equal(code, wc) and (code[np.isinf(dist)] == -1).all()
    only = score_raw(cb[2:3], n_codes[2:3], x, n)  # every distance +inf: every label -1
    assert np.isinf(only[0]).all() and (only[1] == -1).all()
    dist, code = assign_raw(cb, n_codes, x, n, np.zeros(11, np.int32), np.zeros(0, np.int32))
    assert dist.shape == (0,) and code.shape == (0, T)


def test_overflow():
    """Frames of 1e200: every distance overflows to +inf, the code is 0, and there is no NaN anywhere."""
    n_codes = np.array([3, 1], np.int32)
    cb = np.nan_to_num(random_books(n_codes, 4, 2, 80))
    x = np.random.default_rng(81).normal(0, 1, (70, 9, 2))
    x[:5] = 1e200
    x[5, 3] = [-1e200, 1e200]
    n = np.full(70, 9, np.int32)
    start, members = csr([list(range(70)), [0, 5, 6]])
    wd, wc = V.assign(cb, n_codes, x, n, start, members)
    assert np.isinf(wd[:6]).all() and np.isfinite(wd[6:70]).all() and (wc[:5] == 0).all() and wc[5, 3] == 0
    dist, code = assign_raw(cb, n_codes, x, n, start, members)
    same_bits(dist, wd)
    assert np.array_equal(code, wc) and not np.isnan(dist).any()
    score, label = score_raw(cb, n_codes, x, n)
    same_bits(score[:, 0], wd[:70])
    assert not np.isnan(score).any() and (label[:6] == -1).all() and (label[6:] >= 0).all()


def accumulate_case(seed=120):
    """Five codebooks (K = 4, 1, 6, 5, 3 of Kmax = 6) over 90 sequences of 1 .. 30 frames whose scale spans
    eight orders of magnitude: groups of 40, 16, 17, 0 and 5 members in a shuffled order; codebook 3 has
    no member and codebook 4 only members that are skipped."""
    rng = np.random.default_rng(seed)
    N, T, F, K = 90, 30, 3, np.array([4, 1, 6, 5, 3], np.int32)
    x = rng.normal(0, 1, (N, T, F)) * 10.0 ** rng.integers(-4, 5, (N, 1, 1))
    n = rng.integers(1, T + 1, N).astype(np.int32)
    n[80:] = [0, T + 1] * 5
    groups = [rng.permutation(80)[:k].tolist() for k in (40, 16, 17, 0)] + [[80, 81, -1, N, 82]]
    start, members = csr(groups)
    return x, n, K, start, members, rng.normal(0, 1, (5, 6, F))


def test_accumulate_given_codes():
    """Arbitrary given codes; the list order is the order of the sums; a member with one out-of-range
    code is skipped whole; an empty cell and a codebook without valid members are copied bit for bit."""
    x, n, K, start, members, prev = accumulate_case()
    rng = np.random.default_rng(121)
    owner = np.repeat(np.arange(5), np.diff(start))
    code = rng.integers(0, 1 << 20, (len(members), x.shape[1])) % K[owner][:, None]
    code[owner == 2] = np.minimum(code[owner == 2], 4)  # cell 5 of codebook 2 stays empty
    code = code.astype(np.int32)
    dist = rng.uniform(1, 100, len(members)) * 10.0 ** rng.integers(-4, 5, len(members))
    want = V.accumulate(prev, K, x, n, start, members, code, dist)
    assert want[2].tolist() == [40, 16, 17, 0, 0] and want[1][2, 5] == 0 and (want[1][2, :5] > 0).all()
    same_bits(want[0][2, 5], prev[2, 5])
    same_bits(want[0][3:], prev[3:])
    assert want[3][3:].tolist() == [0.0, 0.0] and not want[1][3:].any() and not want[0][0, 4:].any()
    check_accumulate(accumulate_raw(prev, K, x, n, start, members, code, dist), want)
    # the order of the list is the order of the sums: the reference itself gives other bits when permuted
    perm = np.r_[39:-1:-1, 40:len(members)]
    other = V.accumulate(prev, K, x, n, start, members[perm], code[perm], dist[perm])
    assert not np.array_equal(bits(other[0][0]), bits(want[0][0])) and np.array_equal(other[1], want[1])
    check_accumulate(accumulate_raw(prev, K, x, n, start, members[perm], code[perm], dist[perm]), other)
    # one out-of-range code (K and -1), an n_codes of 0: skipped whole
    bad, K2 = code.copy(), K.copy()
    bad[0, n[members[0]] - 1], bad[1, 0] = K[0], -1
    bad[2, n[members[2]]:] = 99  # behind the member's frames: not looked at
    K2[1] = 0
    want2 = V.accumulate(prev, K2, x, n, start, members, bad, dist)
    assert want2[2].tolist() == [38, 0, 17, 0, 0]
    same_bits(want2[0][1], prev[1])
    check_accumulate(accumulate_raw(prev, K2, x, n, start, members, bad, dist), want2)


def test_accumulate_after_assign():
    """dsp_vq_assign's own code and dist as the input, F = 2 and K up to 256."""
    cb, n_codes, x, n, _, start, members, _ = table_case(2)
    cb, x = np.nan_to_num(cb), np.nan_to_num(x)
    dist, code = assign_raw(cb, n_codes, x, n, start, members)
    want = V.accumulate(cb, n_codes, x, n, start, members, code, dist)
    assert want[2][5] == 0 and want[2][4] == 130 and (want[1][8] == 0).any() and (want[1][8] > 0).any()
    check_accumulate(accumulate_raw(cb, n_codes, x, n, start, members, code, dist), want)


def test_accumulate_without_pairs():
    """P = 0 is not "nothing to do" for the re-estimation: every codebook is copied bit for bit, with
    total 0.0, n_valid 0 and cnt 0 (also with no sequences at all)."""
    x, n, K, _, _, prev = accumulate_case()
    none = np.zeros(0, np.int32)
    for xs, ns in ((x, n), (x[:0], n[:0])):
        cen, cnt, nv, total = accumulate_raw(prev, K, xs, ns, np.zeros(6, np.int32), none, np.zeros((0, x.shape[1]), np.int32),
                                             np.zeros(0))
        same_bits(cen, prev)
        assert not cnt.any() and not nv.any() and total.tolist() == [0.0] * 5 and not np.signbit(total).any()
        check_accumulate((cen, cnt, nv, total), V.accumulate(prev, K, xs, ns, np.zeros(6, np.int32), none,
                                                             np.zeros((0, x.shape[1]), np.int32), np.zeros(0)))


def test_accumulate_keeps_a_negative_zero():
    x = np.zeros((3, 2, 1))
    x[0, :, 0], x[1, :, 0], x[2, :, 0] = [1.0, 2.0], [-0.0, -0.0], [3.0, 4.0]
    n = np.array([2, 2, 2], np.int32)
    start, members = csr([[0, 1, 2]])
    code = np.array([[0, 0], [1, 1], [0, 0]], np.int32)
    prev = np.full((1, 3, 1), 7.0)
    got = accumulate_raw(prev, [3], x, n, start, members, code, np.array([-0.0, -0.0, -0.0]))
    check_accumulate(got, V.accumulate(prev, [3], x, n, start, members, code, np.array([-0.0, -0.0, -0.0])))
    assert got[0][0, 1, 0] == 0.0 and np.signbit(got[0][0, 1, 0]) and got[0][0, 0, 0] == 2.5 and np.signbit(got[3][0])


def test_accumulate_pair_chunks():
    """More pairs than one pair chunk holds: at Kmax = 256, F = 8 the plan sums 128 MiB / (256 (4 + 8 * 8) + 4)
    = 7 708 pairs per chunk, and 8 000 pairs drawn with repetition from 50 sequences of 1 .. 3 frames over
    two codebooks put the boundary inside the second group.  The same list run as two calls' worth of
    smaller P: the totals and counts of the two halves add up, and the first half alone is its own call."""
    Kmax, F, T, N = 256, 8, 3, 50
    chunk = (128 << 20) // (Kmax * (4 + 8 * F) + 4)
    sizes = [5000, 3000]
    P = sum(sizes)
    assert chunk == 7708 and sizes[0] < chunk < P
    rng = np.random.default_rng(160)
    x, n = rng.normal(0, 1, (N, T, F)), rng.integers(1, 4, N).astype(np.int32)
    K = np.array([256, 200], np.int32)
    cb = np.nan_to_num(random_books(K, Kmax, F, 161))
    members = rng.integers(0, N, P).astype(np.int32)
    members[rng.choice(P, 40, replace=False)] = np.tile([-1, N], 20)
    members[[chunk - 2, chunk + 1]] = [N, -1]
    members[[chunk - 1, chunk]] = [0, 3]  # valid members on either side of the boundary
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    dist, code = assign_raw(cb, K, x, n, start, members)
    wd, wc = V.assign(cb, K, x, n, start, members)
    same_bits(dist, wd)
    assert np.array_equal(code, wc)
    want = V.accumulate(cb, K, x, n, start, members, code, dist)
    ok = (members >= 0) & (members < N)
    assert want[2].tolist() == [int(ok[:5000].sum()), int(ok[5000:].sum())] and P - 44 <= want[2].sum() <= P - 40
    check_accumulate(accumulate_raw(cb, K, x, n, start, members, code, dist), want)
    # the first 6000 pairs as a call of their own (one chunk): its reference, and group 0 is the same there
    start6 = np.array([0, 5000, 6000], np.int32)
    half = accumulate_raw(cb, K, x, n, start6, members[:6000], code[:6000], dist[:6000])
    check_accumulate(half, V.accumulate(cb, K, x, n, start6, members[:6000], code[:6000], dist[:6000]))
    same_bits(half[0][0], want[0][0])
    assert half[3][0] == want[3][0] and np.array_equal(half[1][0], want[1][0])


def word_sequences(seed, per_class=20):
    """3 classes x 20 sequences of 12 .. 40 frames, F = 2, drawn around five class centres each; the
    classes interleaved, labels 2, 7, 12.  Class 0 takes its frames from three points only, so that at
    n_codes = 8 cells run empty and vq_repair_empty fires."""
    rng = np.random.default_rng(seed)
    means = np.random.default_rng(7).normal(0, 2.0, (3, 5, 2)) * [1.0, 40.0]
    seqs, y = [], []
    for i in range(3 * per_class):
        c, n = i % 3, int(rng.integers(12, 41))
        state = rng.integers(0, 5 if c else 3, n)
        noise = rng.normal(0, 0.5, (n, 2)) * [1.0, 40.0] if c else np.zeros((n, 2))
        seqs.append(means[c, state] + noise)
        y.append(5 * c + 2)
    return seqs, np.array(y)


def pad(seqs):
    n = np.array([len(s) for s in seqs], np.int32)
    out = np.zeros((len(seqs), int(n.max()), seqs[0].shape[1]))
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out, n


@pytest.mark.parametrize("n_codes", (1, 2, 8))
def test_vq_classifier(n_codes):
    from src.models import create_classifier
    from src.pipeline import vq_assign, vq_score
    seqs, y = word_sequences(140)
    clf = create_classifier('vq', n_codes=n_codes, n_iter=4).fit(seqs, y)
    frames = np.concatenate(seqs)
    mean, std = frames.mean(axis=0), frames.std(axis=0)
    X, n = pad([(s - mean) / std for s in seqs])
    classes, codes = np.unique(y, return_inverse=True)
    cb, cnt, totals, repairs = V.fit(X, n, codes, n_codes, n_iter=4, eps=0.01)
    assert (repairs > 0) == (n_codes == 8)  # class 0 has three distinct frames
    assert clf.totals_.shape == totals.shape and clf.n_iter_ == len(totals) and clf.codebooks_.shape == (3, n_codes, 2)
    same_bits(clf.codebooks_, cb)
    same_bits(clf.totals_, totals)
    assert np.array_equal(clf.counts_, cnt) and clf.counts_.sum() == n.sum()
    queries, yq = word_sequences(141)
    q, nq = pad([(s - mean) / std for s in queries])
    sizes = np.full(3, n_codes, np.int32)
    ws, wl = V.score(cb, sizes, q, nq)
    same_bits(clf.score_samples(queries), ws / nq.astype(np.float64)[:, None])
    pred = clf.predict(queries)
    assert np.array_equal(pred, classes[wl])
    assert clf.evaluate(queries, yq)["accuracy"] == float(np.mean(classes[wl] == yq)) > 0.9
    # the device surface under it
    score, label = vq_score(cb, sizes, q, nq, with_labels=True)
    same_bits(score.cpu().numpy(), ws)
    assert np.array_equal(label.cpu().numpy(), wl)
    assign = np.where(np.arange(len(y)) % 5 == 0, -1, codes)
    dist, code, start, members = vq_assign(cb, sizes, X, n, assign=assign)
    start, members = start.cpu().numpy(), members.cpu().numpy()
    wd, wc = V.assign(cb, sizes, X, n, start, members)
    same_bits(dist.cpu().numpy(), wd)
    assert np.array_equal(code.cpu().numpy(), wc) and len(members) == int((assign >= 0).sum())
    only = vq_assign(cb, sizes, X, n, groups=(start, members), with_codes=False)
    assert only[1] is None
    same_bits(only[0].cpu().numpy(), wd)


def test_a_class_with_too_few_frames():
    from src.models import create_classifier
    seqs, y = word_sequences(140, per_class=2)
    with pytest.raises(ValueError):
        create_classifier('vq', n_codes=256).fit([s[:40] for s in seqs], y)


def test_assign_and_accumulate_in_a_graph():
    """dsp_vq_assign followed by dsp_vq_accumulate (no allocation, no sync, the counts zeroed by a
    kernel) captured in a single-stream graph and replayed twice: the eager calls' bits."""
    import torch
    from src import _hip
    lib = _hip.lib()
    cb, n_codes, x, n, _, start, members, (wd, wc) = table_case(2)
    cb, x = np.nan_to_num(cb), np.nan_to_num(x)
    want = V.accumulate(cb, n_codes, x, n, start, members, wc, wd)
    (N, T, F), (C, Kmax), P = x.shape, cb.shape[:2], len(members)
    t = [_dev(cb, torch.float64), _dev(n_codes, torch.int32), _dev(x, torch.float64), _dev(n, torch.int32),
         _dev(start, torch.int32), _dev(members, torch.int32)]
    dist = torch.empty(P, dtype=torch.float64, device="cuda")
    code = torch.empty((P, T), dtype=torch.int32, device="cuda")
    out = [torch.empty((C, Kmax, F), dtype=torch.float64, device="cuda"), torch.empty((C, Kmax), dtype=torch.int32, device="cuda"),
           torch.empty(C, dtype=torch.int32, device="cuda"), torch.empty(C, dtype=torch.float64, device="cuda")]
    ws, nbytes = _workspace(C, N, P, T, F, Kmax)
    p = [_hip.ptr(v) for v in t]

    def call():
        rc = lib.dsp_vq_assign(p[0], p[1], C, Kmax, p[2], p[3], N, T, F, p[4], p[5], P, _hip.ptr(dist), _hip.ptr(code),
                               _hip.ptr(ws), nbytes, _hip.stream_handle())
        assert rc == 0
        rc = lib.dsp_vq_accumulate(p[0], p[1], C, Kmax, p[2], p[3], N, T, F, p[4], p[5], P, _hip.ptr(code), _hip.ptr(dist),
                                   *[_hip.ptr(o) for o in out], _hip.ptr(ws), nbytes, _hip.stream_handle())
        assert rc == 0

    call()
    torch.cuda.synchronize()
    check_accumulate([o.cpu().numpy() for o in out], want)
    assert np.array_equal(code.cpu().numpy(), wc)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        for o in out + [dist, code]:
            o.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        check_accumulate([o.cpu().numpy() for o in out], want)
        same_bits(dist.cpu().numpy(), wd)
        assert np.array_equal(code.cpu().numpy(), wc)


def _write_wav(path, data, width=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(width)
        w.setframerate(44100)
        w.writeframes(np.ascontiguousarray(data).tobytes())


def test_compare_with_vq(tmp_path):
    """compare(hmm=True, vq=True): the rows of compare(hmm=True) unchanged, plus 'VQ' beside 'HMM' whose
    sequence accuracy is the restatement's on the same split (3 words x 5 synthetic clips)."""
    import compare_feature_methods as cfm
    from sklearn.model_selection import train_test_split
    from src.synth import make_clip
    for c in range(3):
        d = tmp_path / ("w%d" % c)
        d.mkdir()
        for j in range(5):
            _write_wav(d / ("s%d.wav" % j), make_clip(3000 + 10 * c + j, n_samples=36000 + 1013 * j, label=c, n_classes=3))
    base = cfm.compare(str(tmp_path), hmm=True)
    res = cfm.compare(str(tmp_path), hmm=True, vq=True)
    assert list(base)[-1] == "HMM" and list(res) == list(base) + ["VQ"]
    assert {k: res[k] for k in base} == base
    row = res["VQ"]
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
    cb, _, _, _ = V.fit(b, lb, codes, 16, n_iter=10, eps=0.01)
    _, label = V.score(cb, np.full(len(cb), 16, np.int32), a, la)
    assert row["sequence"] == float(np.mean(classes[label] == y[te]))
    with pytest.raises(ValueError):
        cfm.compare(str(tmp_path), vq=True, lpc=7)
