"""numpy restatements of the DTW definition in include/dsp_audiorec.h -- the test reference of
csrc/dtw.hip (nothing else on the machine computes a DTW).  Two independent forms that must agree
bit for bit: a scalar triple loop (dtw_scalar) and one vectorised over the pairs, looping over the
cells with arrays over (Nq, Nr) (dtw_pairwise).  Plus the top-k and the vote of dsp_dtw_knn.

  c(i,j) = sum_f (a[i,f] - b[j,f])^2     f ascending, each product and each sum rounded
  D(0,0) = c(0,0);  D(i,j) = c(i,j) + min(D(i-1,j), D(i,j-1), D(i-1,j-1)), +inf outside grid / band
  dtw    = sqrt(D(n-1, m-1));  band: |i - j| <= max(window, |n - m|) for window >= 0
A length < 1 or greater than the padded width: +inf to everything.
"""
import functools
import math

import numpy as np

INF = np.inf


def dtw_scalar(a, b, window=-1):
    """One pair: a [n, F], b [m, F] (unpadded) -> float64.  Python floats are IEEE doubles, so the
    loop below is the definition cell by cell, each product and each sum rounded once."""
    a, b = np.asarray(a, np.float64).tolist(), np.asarray(b, np.float64).tolist()
    n, m = len(a), len(b)
    w = max(int(window), abs(n - m)) if window is not None and window >= 0 else None
    D = [[INF] * m for _ in range(n)]
    for i in range(n):
        ai = a[i]
        for j in range(m):
            if w is not None and abs(i - j) > w:
                continue
            bj = b[j]
            c = None
            for x, y in zip(ai, bj):
                t = x - y
                c = t * t if c is None else c + t * t
            if i == 0 and j == 0:
                D[i][j] = c
                continue
            best = INF
            if i > 0:
                best = min(best, D[i - 1][j])
            if j > 0:
                best = min(best, D[i][j - 1])
            if i > 0 and j > 0:
                best = min(best, D[i - 1][j - 1])
            D[i][j] = c + best
    return np.float64(math.sqrt(D[n - 1][m - 1]))


def dtw_pairwise(a, len_a, b, len_b, window=-1):
    """Padded a [Nq, Tq, F], b [Nr, Tr, F] with lengths -> float64 [Nq, Nr]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    la, lb = np.asarray(len_a, np.int64), np.asarray(len_b, np.int64)
    (Nq, Tq, F), (Nr, Tr, _) = a.shape, b.shape
    ok_a, ok_b = (la >= 1) & (la <= Tq), (lb >= 1) & (lb <= Tr)
    n = np.where(ok_a, la, 1)[:, None]
    m = np.where(ok_b, lb, 1)[None, :]
    if window is not None and window >= 0:
        w = np.maximum(int(window), np.abs(n - m))
    else:
        w = np.full((Nq, Nr), Tq + Tr)
    nmax, mmax = int(n.max()), int(m.max())
    out = np.full((Nq, Nr), INF)
    prev = np.full((mmax, Nq, Nr), INF)  # row i - 1
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(nmax):
            cur = np.full((mmax, Nq, Nr), INF)
            ai = a[:, i, :]
            for j in range(mmax):
                bj = b[:, j, :]
                t = ai[:, None, 0] - bj[None, :, 0]
                c = t * t
                for f in range(1, F):
                    t = ai[:, None, f] - bj[None, :, f]
                    c = c + t * t
                if i == 0 and j == 0:
                    d = c
                else:
                    best = prev[j] if i > 0 else np.full((Nq, Nr), INF)
                    if j > 0:
                        best = np.minimum(best, cur[j - 1])
                        if i > 0:
                            best = np.minimum(best, prev[j - 1])
                    d = c + best
                live = (i < n) & (j < m) & (np.abs(i - j) <= w)
                cur[j] = np.where(live, d, INF)
                end = (i == n - 1) & (j == m - 1)
                out = np.where(end, cur[j], out)
            prev = cur
    out = np.sqrt(out)
    out[~ok_a, :] = INF
    out[:, ~ok_b] = INF
    return out


def dtw_wavefront(a, b, window=-1):
    """One pair again, a [n, F], b [m, F], vectorised over the anti-diagonals (whose cells do not
    depend on each other): the same operations per cell, fast enough for the longest sequences of the
    plan.  tests/test_dtw_host.py holds it to the two forms above bit for bit."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n, m = len(a), len(b)
    t = a[:, None, 0] - b[None, :, 0]
    C = t * t
    for f in range(1, a.shape[1]):
        t = a[:, None, f] - b[None, :, f]
        C = C + t * t
    w = max(int(window), abs(n - m)) if window is not None and window >= 0 else n + m
    D = np.full((n + 1, m + 1), INF)  # D[i + 1, j + 1] = D(i, j); the border is outside the grid
    D[0, 0] = 0.0  # seen by cell (0, 0) only: D(0,0) = c(0,0) + 0
    for s in range(n + m - 1):
        i = np.arange(max(0, s - m + 1), min(n - 1, s) + 1)
        j = s - i
        keep = np.abs(i - j) <= w
        i, j = i[keep], j[keep]
        best = np.minimum(np.minimum(D[i, j + 1], D[i + 1, j]), D[i, j])
        D[i + 1, j + 1] = C[i, j] + best
    return np.sqrt(D[n, m])


def knn_from_dist(dist, k, labels=None, self_offset=-1):
    """dsp_dtw_knn's selection on a distance matrix [Nq, Nr]: ascending (distance, index), only finite
    distances, row self_offset + q excluded -> (idx int32 [Nq,k], dist [Nq,k], pred int32 [Nq] or None).
    The vote is uniform; the smallest label among the most frequent wins; -1 without a neighbour."""
    dist = np.asarray(dist, np.float64)
    Nq, Nr = dist.shape
    idx = np.full((Nq, k), -1, np.int32)
    out = np.full((Nq, k), INF)
    pred = np.full(Nq, -1, np.int32) if labels is not None else None
    for q in range(Nq):
        cand = [(dist[q, r], r) for r in range(Nr)
                if np.isfinite(dist[q, r]) and not (self_offset >= 0 and r == self_offset + q)]
        cand.sort()
        for j, (d, r) in enumerate(cand[:k]):
            idx[q, j], out[q, j] = r, d
        if labels is not None and cand:
            labs = [int(labels[r]) for _, r in cand[:k]]
            counts = {}
            for v in labs:
                counts[v] = counts.get(v, 0) + 1
            top = max(counts.values())
            pred[q] = min(v for v, c in counts.items() if c == top)
    return idx, out, pred


def pad(seqs, T=None):
    """A list of [n_i, F] arrays -> (padded [N, T, F] zeros after each sequence, lengths int32)."""
    n = np.array([len(s) for s in seqs], np.int32)
    T = int(T or n.max())
    out = np.zeros((len(seqs), T, np.asarray(seqs[0]).shape[1]))
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out, n


FORCED_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 70)


def case(Nq, Nr, T, F, seed):
    """The pairwise table's inputs: lengths forced to FORCED_LENGTHS (those <= T) on both sides, the
    rest random in [1, T]; the padding holds other values than zero, which nothing may read as a frame."""
    rng = np.random.default_rng(seed)

    def side(N):
        forced = [v for v in FORCED_LENGTHS if v <= T][:N]
        n = np.concatenate([forced, rng.integers(1, T + 1, N - len(forced))]).astype(np.int32)
        rng.shuffle(n)
        x = rng.normal(0.0, 1.0, (N, T, F)) * rng.uniform(0.5, 2.0, F)
        return x, n

    a, la = side(Nq)
    b, lb = side(Nr)
    return a, la, b, lb


@functools.lru_cache(maxsize=None)
def table_case(F):
    """The pairwise case table's inputs for F channels: Nq = 19, Nr = 37 (no multiple of a tile or a
    wave), T = 70, every forced length on both sides.  Treat the arrays as read-only."""
    a, la, b, lb = case(19, 37, 70, F, seed=40 + F)
    for v in FORCED_LENGTHS:
        assert v in la and v in lb
    return a, la, b, lb


TABLE_F = (1, 2, 3, 8)
TABLE_WINDOWS = (-1, 0, 3, 100)
