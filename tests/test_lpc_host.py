"""CPU tests of the LPC definition's restatement (tests/lpc_reference.py) against independent forms, of
the host side of dsp_lpc_workspace_bytes / dsp_lpc_autocorr / dsp_lpc_solve, and of the Python argument
checks."""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest

import lpc_reference as R
import pitch_reference as P

L = 1102


@functools.lru_cache(maxsize=None)
def frames_r():
    """r(0..32) of 6 synthetic clips x 4 positions x (unwindowed, Q15 Hamming): 48 integer rows."""
    from src.pipeline import lpc_window
    from src.synth import make_clip
    ham = lpc_window("hamming", L)
    rows = []
    for i in range(6):
        x = make_clip(7 + i, label=i % 10)
        y = x.astype(np.int64) - P.centre(x)
        for s in (3000, 9000, 14000, 20000):
            f = y[s:s + L]
            for table in (None, ham):
                rows.append(R.autocorr(R.apply_window(f, table), 32))
    return rows


def levinson_fraction(r, p):
    """The same recursion in exact rationals on the same integers -> (a, k, err, reached)."""
    Rr = [Fraction(int(v)) for v in r]
    a, k, E, m = [Fraction(0)] * (p + 1), [Fraction(0)] * (p + 1), Rr[0], 0
    for i in range(1, p + 1):
        if not E > 0:
            break
        ki = (Rr[i] - sum(a[j] * Rr[i - j] for j in range(1, i))) / E
        if not abs(ki) < 1:
            break
        a = [a[j] - ki * a[i - j] if 1 <= j < i else (ki if j == i else a[j]) for j in range(p + 1)]
        k[i] = ki
        E, m = E * (1 - ki * ki), i
    return a[1:], k[1:], E, m


@pytest.mark.parametrize("p", (12, 32))
def test_levinson_against_exact_rationals(p):
    """a, k and err against the exact values, each error relative to the largest magnitude of its vector
    (a coefficient that cancels to nearly zero has no relative precision of its own: element-wise the
    worst is 9e-10).  A wrong index or sign moves a value by 1e-2 of that scale or more; rounding stays
    near 2e-12."""
    worst = 0.0
    for r in frames_r():
        a, k, err, m, _ = R.solve_row(r[:p + 1], p, 0)
        ea, ek, eerr, em = levinson_fraction(r[:p + 1], p)
        assert m == em == p
        for got, want in ((a, ea), (k, ek), ([err], [eerr])):
            scale = max(abs(w) for w in want)
            worst = max([worst] + [abs(float((Fraction(float(g)) - w) / scale)) for g, w in zip(got, want)])
    print("worst relative error against the rational recursion, p = %d: %.3g" % (p, worst))
    assert worst <= 1e-9


@pytest.mark.parametrize("p", (12, 32))
def test_cepstrum_against_pole_power_sums(p):
    worst = 0.0
    for r in frames_r():
        a, _, _, m, cep = R.solve_row(r[:p + 1], p, 24)
        assert m == p
        z = np.roots(np.concatenate([[1.0], -a]))
        assert (np.abs(z) < 1).all()  # |k| < 1 throughout: minimum phase
        want = np.array([np.sum(z ** n).real / n for n in range(1, 25)])
        worst = max(worst, float(np.abs(cep - want).max()))
    print("worst absolute error against the pole power sums, p = %d: %.3g" % (p, worst))
    assert worst <= 1e-10


def test_known_answers_and_stop_rules():
    a, k, err, m, cep = R.solve_row([2 ** (20 - j) for j in range(9)], 8, 4)
    assert a.tolist() == [0.5] + [0.0] * 7 and k.tolist() == [0.5] + [0.0] * 7
    assert (err, m) == (786432.0, 8) and cep.tolist() == [0.5, 0.125, 1.0 / 24.0, 0.015625]
    for r, want_err in (([1, 1, 1, 1, 1], 1.0), ([1, 2, 0], 1.0), ([-3, 1, 1], -3.0), ([0, 0, 0], 0.0)):
        p = len(r) - 1
        a, k, err, m, cep = R.solve_row(r, p, 5)
        assert m == 0 and err == want_err and not a.any() and not k.any() and not cep.any(), r
    # a stop in the middle keeps the orders reached: r = (4, 2, 4) has k1 = 0.5, then k2 = 1
    a, k, err, m, cep = R.solve_row([4, 2, 4, 0], 3, 3)
    assert (m, err) == (1, 3.0) and a.tolist() == [0.5, 0.0, 0.0] and cep.tolist() == [0.5, 0.125, 1.0 / 24.0]
    # the conversion is round to nearest even
    assert R.solve_row([2 ** 53 + 1, 0], 1, 0)[2] == 2.0 ** 53 and R.solve_row([2 ** 53 + 3, 0], 1, 0)[2] == 2.0 ** 53 + 4
    assert R.solve_row([-(2 ** 53) - 1, 0], 1, 0)[2:4] == (-(2.0 ** 53), 0)
    assert R.solve_row([2 ** 60, 2 ** 53 + 1], 1, 1)[0].tolist() == [2.0 ** -7]
    assert R.solve_row([2 ** 62 + 2 ** 9 + 1, 0], 1, 0)[2] == 2.0 ** 62 + 2.0 ** 10
    # batched: identical rows, mixed stop orders
    a, k, err, m, cep = R.solve([[4, 2, 4, 0], [0, 0, 0, 0], [8, 4, 2, 1]], 3, 2)
    assert m.tolist() == [1, 0, 3] and err.tolist() == [3.0, 0.0, 6.0] and a[2].tolist() == [0.5, 0.0, 0.0]


def test_window_table_and_rounding():
    from src.pipeline import create_window, lpc_window
    ham = lpc_window("hamming", L)
    assert ham.dtype == np.int32 and ham.shape == (L,) and (ham.min(), ham.max()) == (2621, 32768)
    assert np.array_equal(ham, R.q15_window(create_window("hamming", L))) and lpc_window("rectangular", L) is None
    assert lpc_window("hanning", 5).tolist() == [0, 16384, 32768, 16384, 0]
    with pytest.raises(ValueError):
        lpc_window("kaiser", 8)
    # the shift is a floor: halves go up, on both sides of zero
    f = np.array([-3, -1, -1, -1, 1, 3, -65535, 65535, -7], np.int64)
    w = np.array([16384, 16384, 16383, 16385, 16384, 16384, 32768, 32768, 1], np.int32)
    assert R.apply_window(f, w).tolist() == [-1, 0, 0, -1, 1, 2, -65535, 65535, 0]
    assert R.apply_window(f, w).tolist() == [int(np.floor(int(a) * int(b) / 32768.0 + 0.5)) for a, b in zip(f, w)]
    # entries outside [0, 32768] are clamped; no table is the identity
    assert R.apply_window([-9, 9, 100, -100], [-5, 40000, -(2 ** 31), 2 ** 31 - 1]).tolist() == [0, 9, 0, -100]
    assert R.apply_window(f, None).tolist() == f.tolist() == R.apply_window(f, [32768] * 9).tolist()
    # r of a short known frame, and of its zero-padded tail
    assert R.autocorr([1, -2, 3, 0, 0], 3).tolist() == [14, -8, 3, 0]
    x = np.array([5, -3, 8, 1, -6, 2, 7, -4], np.int16)
    r = R.autocorr_clip(x, 1, 7, 2, 4, 3, 2, None)  # c = 1: y = 4 -4 7 0 -7 1 6 -5; frames y[1:5], y[4:7] + 0
    assert P.centre(x) == 1 and r.tolist() == [[16 + 49 + 49, -28, -49], [49 + 1 + 36, -7 + 6, -42]]


def test_abi_argument_checks():
    """Every plan bound, the NULL checks, B = 0 and n = 0, answered on the host before any launch."""
    from src import _hip
    lib = _hip.load_library()
    wb = lib.dsp_lpc_workspace_bytes
    assert wb(10, 44100, 1102, 441, 12) > 0 and wb(0, 1, 2, 1, 1) > 0 and wb(1, 5, 4096, 1, 32) > 0 and wb(1, 5, 33, 1, 32) > 0
    for args in ((10, 44100, 1, 441, 1), (10, 44100, 4097, 441, 12), (10, 44100, 1102, 441, 0), (10, 44100, 1102, 441, 33),
                 (10, 44100, 32, 441, 32), (10, 44100, 2, 1, 2), (10, 44100, 1102, 0, 12), (-1, 44100, 1102, 441, 12),
                 (10, 0, 1102, 441, 12)):
        assert wb(*args) == 0, args
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(B=4, L=1102, S=441, order=12, window=p, ptrs=(p,) * 6, stride=0, ld=8, ws=p, nws=1 << 20, max_len=4000):
        pcm, off, se, nf, st, r = ptrs
        return lib.dsp_lpc_autocorr(pcm, off, B, max_len, L, S, order, window, se, nf, st, stride, r, ld, ws, nws, None)

    for bad in (dict(L=1), dict(L=4097), dict(order=0), dict(order=33), dict(L=12, order=12), dict(S=0), dict(ld=0),
                dict(stride=5), dict(B=-1), dict(max_len=0)):
        assert call(**bad) == _hip.DSP_ERR_ARGS, bad
    for k in range(6):
        assert call(ptrs=tuple(None if i == k else p for i in range(6))) == _hip.DSP_ERR_ARGS, k
    assert call(ws=None, nws=0) == _hip.DSP_ERR_WORKSPACE and call(nws=wb(4, 4000, 1102, 441, 12) - 1) == _hip.DSP_ERR_WORKSPACE
    assert call(B=0) == _hip.DSP_OK and call(B=0, ptrs=(None,) * 6, window=None, ws=None, nws=0) == _hip.DSP_OK
    assert call(B=0, stride=19) == _hip.DSP_OK

    def solve(n=5, order=12, Q=12, ptrs=(p,) * 6):
        r, a, k, err, reached, cep = ptrs
        return lib.dsp_lpc_solve(r, n, order, Q, a, k, err, reached, cep, None)

    for bad in (dict(order=0), dict(order=33), dict(Q=-1), dict(Q=65), dict(n=-1)):
        assert solve(**bad) == _hip.DSP_ERR_ARGS, bad
    for k in range(6):  # k = 5: cep NULL with Q > 0
        assert solve(ptrs=tuple(None if i == k else p for i in range(6))) == _hip.DSP_ERR_ARGS, k
    assert solve(n=0) == _hip.DSP_OK and solve(n=0, ptrs=(None,) * 6) == _hip.DSP_OK and solve(n=0, Q=0, order=32) == _hip.DSP_OK
    assert solve(n=0, order=33) == _hip.DSP_ERR_ARGS


def test_python_argument_checks_without_a_device():
    import compare_feature_methods as cfm
    from src.dataset import PCMDataset
    from src.pipeline import LpcAnalyzer, lpcc_statistics
    an = LpcAnalyzer(1102, 441)
    assert (an.L, an.S, an.p, an.Q) == (1102, 441, 12, 12) and np.array_equal(an.table, R.q15_window(np.hamming(1102)))
    assert LpcAnalyzer(64, 16, 8, 0, "rectangular").table is None and an.frames(1102) == 1 and an.frames(1103) == 2
    assert LpcAnalyzer(33, 7, 32, 64).frames(48) == 4
    for bad in (dict(frame_length=1), dict(frame_length=4097), dict(frame_length=100.5), dict(frame_shift=0), dict(order=0),
                dict(order=33), dict(frame_length=12, order=12), dict(order=True), dict(n_cep=-1), dict(n_cep=65),
                dict(n_cep=2.5), dict(window_type="kaiser")):
        kw = dict(frame_length=1102, frame_shift=441)
        kw.update(bad)
        with pytest.raises(ValueError):
            LpcAnalyzer(**kw)
    with pytest.raises(ValueError):
        an(np.zeros((2, 4000), np.int32), {"rows": None})  # int32 samples, refused before any device is asked for
    ds = PCMDataset.__new__(PCMDataset)  # the argument check comes before the first use of the dataset
    for bad in (-1, 65, 2.5, True):
        with pytest.raises(ValueError):
            ds.extract_both(1102, 441, lpc=bad)
    # compare: the sequence kernels take F <= 8, checked before the data is touched
    for kw in (dict(hmm=True, lpc=7), dict(dtw=True, lpc=6, pitch=True), dict(dtw_template=True, lpc=64), dict(lpc=-1),
               dict(lpc=65)):
        with pytest.raises(ValueError):
            cfm.compare("/nonexistent", **kw)
    cep = np.arange(24, dtype=np.float64).reshape(2, 4, 3) ** 2
    got = lpcc_statistics(cep, [3, 0])
    assert got.shape == (2, 6) and np.array_equal(got[0], R.lpcc_stats(cep[0], 3)) and not got[1].any()
    assert np.array_equal(got[0, :3], np.mean(cep[0, :3], axis=0)) and np.array_equal(got[0, 3:], np.std(cep[0, :3], axis=0))
