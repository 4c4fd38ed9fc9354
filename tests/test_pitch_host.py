"""CPU tests of the pitch-track definition (tests/pitch_reference.py), of the host side of
dsp_pitch_workspace_bytes / dsp_pitch_track, and of PitchTracker's argument checks."""
import ctypes

import numpy as np
import pytest

import pitch_reference as P


@pytest.mark.parametrize("period", (37, 110, 200, 441))
def test_pulse_train_returns_its_period(period):
    L = 1102
    x = np.zeros(3 * L, np.int16)
    x[::period] = 1200
    lag, peak, r0 = P.track_clip(x, 0, len(x), 2, L, 441, 20, 735)
    assert (lag == period).all()  # 2 P, 3 P ... tie or fall short: the smallest lag of the maximum wins
    assert (peak > 0).all() and (peak <= r0).all()
    assert P.voiced(peak, r0).all() and (P.f0(lag, True, 44100) == 44100.0 / period).all()


def test_tie_rule():
    x = P.tie_clip()
    assert int(x.astype(np.int64).sum()) == 0 and P.centre(x) == 0
    f = P.frame(x.astype(np.int64), 0, len(x), 0, 1102, 441)
    assert [P.autocorr(f, t) for t in (200, 300, 500)] == [1000000] * 3 and P.autocorr(f, 0) == 3000000
    assert max(P.autocorr(f, t) for t in range(1, 1102)) == 1000000
    assert P.track_frame(f, 110, 735) == (200, 1000000, 3000000)
    assert P.track_frame(f, 201, 735) == (300, 1000000, 3000000)
    assert P.track_frame(f, 301, 735) == (500, 1000000, 3000000)
    assert P.track_frame(f, 501, 735) == (501, 0, 3000000)  # nothing left: the first lag of the range


def test_centre_rounds_half_up():
    c = lambda v: P.centre(np.array(v, np.int16))
    assert c([1, 2]) == 2 and c([-1, -2]) == -1 and c([0, 1]) == 1 and c([0, -1]) == 0  # exact halves go up
    assert c([1, 1, 2]) == 1 and c([1, 2, 2]) == 2 and c([-1, -1, -2]) == -1 and c([-1, -2, -2]) == -2
    assert c([-32768] * 7) == -32768 and c([32767] * 5) == 32767 and c([-3]) == -3 and c([0, 0, 0]) == 0
    assert c([-7, 2]) == -2 and c([-5, 0, 0, 0]) == -1 and c([-6, 0, 0, 0]) == -1 and c([-7, 0, 0, 0]) == -2
    rng = np.random.default_rng(0)
    for _ in range(200):
        x = rng.integers(-32768, 32768, rng.integers(1, 40)).astype(np.int16)
        assert P.centre(x) == int(np.floor(x.astype(np.float64).sum() / len(x) + 0.5))  # small sums: exact in fp64


def test_last_frame_is_zero_padded():
    rng = np.random.default_rng(1)
    x = rng.integers(-3000, 3000, 400).astype(np.int16)
    L, S, st, en = 100, 37, 13, 250
    nf = P.frame_count(en - st, L, S)
    assert nf == 5 and st + (nf - 1) * S + L > en
    y = x.astype(np.int64) - P.centre(x)
    last = P.frame(y, st, en, nf - 1, L, S)
    k = en - (st + (nf - 1) * S)
    assert 0 < k < L and np.array_equal(last[:k], y[en - k:en]) and not last[k:].any()
    lag, peak, r0 = P.track_clip(x, st, en, nf, L, S, 5, 60)
    assert r0[-1] == int((y[en - k:en] ** 2).sum())
    want = max((int(np.dot(y[en - k:en - t], y[en - k + t:en])), -t) for t in range(5, 61))
    assert (int(peak[-1]), -int(lag[-1])) == want
    for t in range(nf):  # the batched np.dot against one np.dot per lag
        f = P.frame(y, st, en, t, L, S)
        r = [P.autocorr(f, tau) for tau in range(5, 61)]
        assert (int(lag[t]), int(peak[t]), int(r0[t])) == (5 + int(np.argmax(r)), max(r), P.autocorr(f, 0))
    assert P.frame_count(100, 100, 37) == 1 and P.frame_count(101, 100, 37) == 2 and P.frame_count(5, 100, 37) == 1
    assert P.track_frame(np.zeros(64, np.int64), 7, 20) == (7, 0, 0)


def test_voicing_and_f0():
    peak = np.array([3, 2, 0, -5, 30, 1 << 52])
    r0 = np.array([10, 10, 0, 10, 100, 1 << 53])
    assert P.voiced(peak, r0).tolist() == [True, False, False, False, True, True]
    assert P.voiced(peak, r0, 1, 1).tolist() == [False] * 6
    f = P.f0(np.array([100, 147, 0]), np.array([True, True, False]), 44100)
    assert f.tolist() == [441.0, 300.0, 0.0]
    assert P.f0_stats([100.0, 0.0, 300.0], [True, False, True]).tolist() == [200.0, 100.0, 300.0, 100.0, 200.0]
    assert not P.f0_stats([5.0], [False]).any()


def test_abi_argument_checks():
    """The plan's bounds, the NULL checks and B = 0, answered on the host before any launch."""
    from src import _hip
    lib = _hip.load_library()
    wb = lib.dsp_pitch_workspace_bytes
    assert wb(10, 44100, 1102, 441, 110, 735) > 0 and wb(0, 1, 2, 1, 1, 1) > 0 and wb(1, 5, 4096, 1, 1, 4095) > 0
    for args in ((10, 44100, 1, 441, 1, 1), (10, 44100, 4097, 441, 110, 735), (10, 44100, 1102, 441, 0, 735),
                 (10, 44100, 1102, 441, 110, 1102), (10, 44100, 1102, 441, 736, 735), (10, 44100, 1102, 0, 110, 735),
                 (-1, 44100, 1102, 441, 110, 735), (10, 0, 1102, 441, 110, 735)):
        assert wb(*args) == 0, args
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(B=4, L=1102, lo=110, hi=735, ptrs=(p,) * 8, stride=0, ld=8, ws=p, nws=1 << 20, max_len=4000):
        pcm, off, se, nf, st, lag, peak, r0 = ptrs
        return lib.dsp_pitch_track(pcm, off, B, max_len, L, 441, lo, hi, se, nf, st, stride, lag, peak, r0, ld, ws, nws, None)

    for bad in (dict(L=1), dict(L=4097), dict(lo=0), dict(hi=1102), dict(lo=736), dict(ld=0), dict(stride=5),
                dict(B=-1), dict(max_len=0)):
        assert call(**bad) == _hip.DSP_ERR_ARGS, bad
    for k in range(8):
        assert call(ptrs=tuple(None if i == k else p for i in range(8))) == _hip.DSP_ERR_ARGS, k
    assert call(ws=None, nws=0) == _hip.DSP_ERR_WORKSPACE and call(nws=wb(4, 4000, 1102, 441, 110, 735) - 1) == _hip.DSP_ERR_WORKSPACE
    assert call(B=0) == _hip.DSP_OK and call(B=0, ptrs=(None,) * 8, ws=None, nws=0) == _hip.DSP_OK
    assert call(B=0, stride=19) == _hip.DSP_OK


def test_pitch_tracker_validates_without_a_device():
    from src.pipeline import PitchTracker, f0_statistics
    t = PitchTracker(1102, 441, 44100)
    assert (t.lag_min, t.lag_max, t.vnum, t.vden) == (110, 735, 3, 10) == P.lag_range(44100, 1102) + (3, 10)
    assert (PitchTracker(64, 16, 44100).lag_min, PitchTracker(64, 16, 44100).lag_max) == (63, 63)
    t = PitchTracker(256, 64, 8000, f0_min=50.0, f0_max=9000.0, voicing=(1, 1))
    assert (t.lag_min, t.lag_max) == (1, 160) and t.frames(256) == 1 and t.frames(257) == 2 and t.frames(321) == 3
    for bad in (dict(frame_length=1), dict(frame_length=4097), dict(frame_length=100.5), dict(frame_shift=0),
                dict(sample_rate=0), dict(f0_min=0.0), dict(f0_min=500.0), dict(f0_max=float("inf")),
                dict(voicing=(0, 10)), dict(voicing=(11, 10)), dict(voicing=(3, 1025)), dict(voicing=(0.5, 1)),
                dict(voicing=3)):
        kw = dict(frame_length=1102, frame_shift=441, sample_rate=44100)
        kw.update(bad)
        with pytest.raises(ValueError):
            PitchTracker(**kw)
    with pytest.raises(ValueError):
        t(np.zeros((2, 4000), np.int32), {"rows": None})  # int32 samples, refused before any device is asked for
    f0 = np.array([[100.0, 0.0, 300.0], [0.0, 0.0, 0.0]])
    voiced = np.array([[True, False, True], [False, False, False]])
    assert np.array_equal(f0_statistics(f0, voiced), np.stack([P.f0_stats(a, b) for a, b in zip(f0, voiced)]))
