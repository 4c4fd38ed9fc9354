"""The numpy int64 restatement of the pitch-track definition (include/dsp_audiorec.h, dsp_pitch_track):
the only other implementation of it.  Python integers and int64 arrays throughout; every lag is one
np.dot of two int64 slices."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def centre(x):
    """c = floor((2 sum + N) / (2 N)): the clip mean rounded half up, in Python integers."""
    N = len(x)
    s = int(np.sum(np.asarray(x, np.int64)))
    return (2 * s + N) // (2 * N)


def frame_count(n, L, S):
    """frame_signal's frame count for a crop of n samples."""
    if n <= 0:
        return 0
    return 1 if n <= L else -(-(n - L) // S) + 1


def frame(y, st, en, t, L, S):
    """f_t: L samples of the centred clip from st + t S, zeros from en on."""
    f = np.zeros(L, np.int64)
    a = st + t * S
    k = max(0, min(L, en - a))
    f[:k] = y[a:a + k]
    return f


def autocorr(f, tau):
    return int(np.dot(f[:len(f) - tau], f[tau:]))


def track_frame(f, lag_min, lag_max):
    """(lag, peak, r0) of one frame: the smallest lag of the largest r.  Row tau of W is the frame
    from sample tau on with zeros behind it, so W f is autocorr(f, tau) for all the lags in one int64
    np.dot."""
    f = np.asarray(f, np.int64)
    W = sliding_window_view(np.concatenate([f, np.zeros(lag_max, np.int64)]), len(f))[lag_min:lag_max + 1]
    r = np.dot(W, f)
    k = int(np.argmax(r))  # the first maximum
    return lag_min + k, int(r[k]), int(np.dot(f, f))


def track_clip(x, st, en, nf, L, S, lag_min, lag_max):
    """lag int32 [nf], peak int64 [nf], r0 int64 [nf] of one clip."""
    y = np.asarray(x, np.int64) - centre(x)
    lag, peak, r0 = np.zeros(nf, np.int32), np.zeros(nf, np.int64), np.zeros(nf, np.int64)
    for t in range(nf):
        lag[t], peak[t], r0[t] = track_frame(frame(y, st, en, t, L, S), lag_min, lag_max)
    return lag, peak, r0


def track_batch(clips, start_end, n_frames, status, L, S, lag_min, lag_max, ld, fill=(-9, -7, -7)):
    """The arrays dsp_pitch_track leaves in outputs [B, ld] that held ``fill``: frames t >= min(nf, ld)
    and the rows of clips with status & 0xFF != 0 untouched."""
    B = len(clips)
    lag = np.full((B, ld), fill[0], np.int32)
    peak = np.full((B, ld), fill[1], np.int64)
    r0 = np.full((B, ld), fill[2], np.int64)
    for b in range(B):
        if int(status[b]) & 0xFF:
            continue
        k = min(int(n_frames[b]), ld)
        lag[b, :k], peak[b, :k], r0[b, :k] = track_clip(clips[b], int(start_end[b][0]), int(start_end[b][1]), k, L, S,
                                                       lag_min, lag_max)
    return lag, peak, r0


def voiced(peak, r0, vnum=3, vden=10):
    peak, r0 = np.asarray(peak, np.int64), np.asarray(r0, np.int64)
    return (peak > 0) & (vden * peak >= vnum * r0)


def f0(lag, is_voiced, sample_rate):
    lag = np.asarray(lag)
    return np.where(is_voiced, np.float64(sample_rate) / np.maximum(lag, 1).astype(np.float64), 0.0)


def f0_stats(f0_row, voiced_row):
    """mean, std, max, min, median of the voiced frames' f0 (numpy fp64), zeros without one."""
    v = np.asarray(f0_row, np.float64)[np.asarray(voiced_row, bool)]
    if v.size == 0:
        return np.zeros(5)
    return np.array([np.mean(v), np.std(v), np.max(v), np.min(v), np.median(v)])


def lag_range(sample_rate, L, f0_min=60.0, f0_max=400.0):
    lo = min(max(int(sample_rate // f0_max), 1), L - 1)
    hi = min(max(int(sample_rate // f0_min), 1), L - 1)
    return lo, hi


def tie_clip():
    """Three pulses of 1000 at 0, 200, 500 and three of -1000 at 1500 .. 1502 in 2204 samples: c = 0 and,
    for the first frame of 1102, r(200) = r(300) = r(500) = 1 000 000, r0 = 3 000 000."""
    x = np.zeros(2204, np.int16)
    x[[0, 200, 500]] = 1000
    x[[1500, 1501, 1502]] = -1000
    return x
