"""The restatement of the LPC definition (include/dsp_audiorec.h, dsp_lpc_autocorr / dsp_lpc_solve): the
only other implementation of it.  The front half is numpy int64 and Python integers; the back half is
np.float64 scalars, one rounded operation at a time, in the order the header fixes."""
import numpy as np

import pitch_reference as P


def q15_window(w):
    """floor(w * 32768 + 0.5) of an fp64 window as int32; None stays None."""
    if w is None:
        return None
    return np.floor(np.asarray(w, np.float64) * 32768.0 + 0.5).astype(np.int32)


def apply_window(f, table):
    """z[i] = (f[i] * min(max(table[i], 0), 32768) + 16384) >> 15 in int64 (>> of a negative: a floor)."""
    f = np.asarray(f, np.int64)
    if table is None:
        return f.copy()
    w = np.clip(np.asarray(table, np.int64), 0, 32768)
    return (f * w + 16384) >> 15


def autocorr(z, p):
    """r(0 .. p) of one frame, int64."""
    z = np.asarray(z, np.int64)
    return np.array([int(np.dot(z[:len(z) - t], z[t:])) for t in range(p + 1)], np.int64)


def autocorr_clip(x, st, en, nf, L, S, p, table):
    y = np.asarray(x, np.int64) - P.centre(x)
    return np.stack([autocorr(apply_window(P.frame(y, st, en, t, L, S), table), p) for t in range(nf)]) \
        if nf else np.zeros((0, p + 1), np.int64)


def autocorr_batch(clips, start_end, n_frames, status, L, S, p, table, ld, fill=-7):
    """What dsp_lpc_autocorr leaves in r [B, ld, p + 1] that held ``fill``."""
    B = len(clips)
    r = np.full((B, ld, p + 1), fill, np.int64)
    for b in range(B):
        if int(status[b]) & 0xFF:
            continue
        k = min(int(n_frames[b]), ld)
        if k > 0:
            r[b, :k] = autocorr_clip(clips[b], int(start_end[b][0]), int(start_end[b][1]), k, L, S, p, table)
    return r


def to_double(v):
    """(double) of an int64: round to nearest even (Python's int -> float conversion is that)."""
    return np.float64(float(int(v)))


def solve_row(r, p, Q):
    """-> (a [p], k [p], err, reached, cep [Q]) of one row r[0 .. p], np.float64 throughout."""
    f = np.float64
    R = [to_double(v) for v in r]
    a = [f(0.0)] * (p + 1)  # 1-based
    k = [f(0.0)] * (p + 1)
    E, m = R[0], 0
    with np.errstate(all="ignore"):
        for i in range(1, p + 1):
            if not E > 0:
                break
            acc = R[i]
            for j in range(1, i):
                acc = f(acc - f(a[j] * R[i - j]))
            ki = f(acc / E)
            if not abs(ki) < 1:
                break
            new = list(a)
            for j in range(1, i):
                new[j] = f(a[j] - f(ki * a[i - j]))
            new[i] = ki
            a = new
            k[i] = ki
            E = f(E * f(f(1.0) - f(ki * ki)))
            m = i
        c = [f(0.0)] * (Q + 1)
        for n in range(1, Q + 1):
            s = f(0.0)
            for q in range(max(1, n - p), n):
                s = f(s + f(f(f(q) * c[q]) * a[n - q]))
            c[n] = f((a[n] if n <= p else f(0.0)) + f(s / f(n)))
    return np.array(a[1:], f), np.array(k[1:], f), f(E), m, np.array(c[1:], f)


def solve(r, p, Q):
    """r [n, p + 1] -> a [n, p], k [n, p], err [n], reached int32 [n], cep [n, Q]."""
    r = np.asarray(r, np.int64).reshape(-1, p + 1)
    n = len(r)
    a, k, cep = np.zeros((n, p)), np.zeros((n, p)), np.zeros((n, Q))
    err, reached = np.zeros(n), np.zeros(n, np.int32)
    cache = {}
    for i in range(n):
        key = r[i].tobytes()
        if key not in cache:
            cache[key] = solve_row(r[i], p, Q)
        a[i], k[i], err[i], reached[i], cep[i] = cache[key]
    return a, k, err, reached, cep


def lpcc_stats(cep, length):
    """mean then std of each cepstrum over the clip's first ``length`` frames (numpy fp64) -> [2 Q]."""
    cep = np.asarray(cep, np.float64)[:length]
    if len(cep) == 0:
        return np.zeros(2 * cep.shape[1])
    return np.concatenate([np.mean(cep, axis=0), np.std(cep, axis=0)])


def wide_frames(*_):
    """Frames on a plain fallback path: the shipped lag sums run on the vector ALU and have none."""
    return 0
