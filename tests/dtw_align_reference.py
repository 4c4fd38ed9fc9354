"""numpy restatements of the alignment path, the ranges, one DBA update and the medoid rule of
include/dsp_audiorec.h (dsp_dtw_align, dsp_dtw_dba_update) -- the test reference of
csrc/dtw_align.hip.  c, D and the band are tests/dtw_reference.py's.

  path    from (n-1, m-1) back to (0, 0): the predecessor of (i, j) is the first of (i-1, j-1),
          (i-1, j), (i, j-1) whose D equals the minimum of the three (+inf outside grid / band)
  ranges  frame i of a is matched to frames lo[i] .. hi[i] of b; -1 for i >= n and for invalid pairs
Two independent forms of the table and the walk that must agree bit for bit: Python floats and explicit
comparisons in the rule's order (table_scalar, backtrace_scalar), and the anti-diagonal wavefront
table with numpy's first-minimum argmin (table_wavefront, backtrace_wavefront; fast enough for
T = 1024).
"""
import math

import numpy as np

import dtw_reference as R

INF = np.inf


def table_scalar(a, b, window=-1):
    """The full table D [n, m] of one pair (unpadded a [n, F], b [m, F]) as a list of lists of Python
    floats, +inf outside the band: dtw_reference.dtw_scalar's loop, keeping every cell."""
    a, b = np.asarray(a, np.float64).tolist(), np.asarray(b, np.float64).tolist()
    n, m = len(a), len(b)
    w = max(int(window), abs(n - m)) if window is not None and window >= 0 else None
    D = [[INF] * m for _ in range(n)]
    for i in range(n):
        for j in range(m):
            if w is not None and abs(i - j) > w:
                continue
            c = None
            for x, y in zip(a[i], b[j]):
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
    return D


def backtrace_scalar(D):
    """The path of a table (list of lists), ascending from (0, 0): explicit comparisons in the rule's
    order -- diagonal, a-step (i-1, j), b-step (i, j-1)."""
    i, j = len(D) - 1, len(D[0]) - 1
    path = [(i, j)]
    while i > 0 or j > 0:
        dg = D[i - 1][j - 1] if i > 0 and j > 0 else INF
        up = D[i - 1][j] if i > 0 else INF
        lf = D[i][j - 1] if j > 0 else INF
        best = min(dg, up, lf)
        if dg == best:
            i, j = i - 1, j - 1
        elif up == best:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    return np.array(path[::-1], np.int64)


def table_wavefront(a, b, window=-1):
    """The table with its border, D[i + 1, j + 1] = D(i, j), by anti-diagonals
    (dtw_reference.dtw_wavefront, keeping the table)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n, m = len(a), len(b)
    t = a[:, None, 0] - b[None, :, 0]
    C = t * t
    for f in range(1, a.shape[1]):
        t = a[:, None, f] - b[None, :, f]
        C = C + t * t
    w = max(int(window), abs(n - m)) if window is not None and window >= 0 else n + m
    D = np.full((n + 1, m + 1), INF)
    D[0, 0] = 0.0  # seen by cell (0, 0) only
    for s in range(n + m - 1):
        i = np.arange(max(0, s - m + 1), min(n - 1, s) + 1)
        j = s - i
        keep = np.abs(i - j) <= w
        i, j = i[keep], j[keep]
        best = np.minimum(np.minimum(D[i, j + 1], D[i + 1, j]), D[i, j])
        D[i + 1, j + 1] = C[i, j] + best
    D[0, 0] = INF  # outside the grid for the walk
    return D, C


def backtrace_wavefront(D):
    """The path of a bordered table: numpy's argmin over (diagonal, a-step, b-step) returns the first
    minimum, which is the rule."""
    i, j = D.shape[0] - 1, D.shape[1] - 1  # bordered indices of (n-1, m-1)
    path = [(i - 1, j - 1)]
    while i > 1 or j > 1:
        step = int(np.argmin([D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]]))
        i, j = (i - 1, j - 1) if step == 0 else ((i - 1, j) if step == 1 else (i, j - 1))
        path.append((i - 1, j - 1))
    return np.array(path[::-1], np.int64)


def ranges(path, T):
    """(lo, hi) int32 [T] of an ascending path: the b frames matched to each a frame, -1 past a's end."""
    lo, hi = np.full(T, -1, np.int32), np.full(T, -1, np.int32)
    for i, j in path.tolist():
        if lo[i] < 0:
            lo[i] = j
        hi[i] = j
    return lo, hi


def path_of_ranges(lo, hi):
    return np.array([(i, j) for i in range(len(lo)) if lo[i] >= 0 for j in range(lo[i], hi[i] + 1)], np.int64)


def tie_case(F, seed, N=8, T=12):
    """Sequences with values in {0, 1, 2}: many cells of D tie exactly.  The last two are (0, 1, 0) and
    (1, 0, 1) in every channel: at their end cell the a-step and the b-step tie below the diagonal, so
    the pair's path and its swap's differ."""
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(0, 3, (int(n), F)).astype(np.float64) for n in rng.integers(1, T + 1, N)]
    return seqs + [np.repeat(np.array(v, np.float64)[:, None], F, axis=1) for v in ((0, 1, 0), (1, 0, 1))]


def check_path(x, y, window, d2, lo, hi):
    """What the ranges of any valid pair must satisfy, whoever computed them: the three range
    invariants, the band, and that the costs summed along the path, ascending, reproduce D(end) bit
    for bit (addition commutes, so the recurrence is that sum)."""
    n, m = len(x), len(y)
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    assert lo[0] == 0 and hi[n - 1] == m - 1 and (lo[n:] == -1).all() and (hi[n:] == -1).all()
    assert (hi[:n - 1] <= lo[1:n]).all() and (lo[1:n] <= hi[:n - 1] + 1).all() and (lo[:n] <= hi[:n]).all()
    path = path_of_ranges(lo, hi)
    if window is not None and window >= 0:
        assert (np.abs(path[:, 0] - path[:, 1]) <= max(window, abs(n - m))).all()
    t = x[path[:, 0], 0] - y[path[:, 1], 0]
    c = t * t
    for f in range(1, x.shape[1]):
        t = x[path[:, 0], f] - y[path[:, 1], f]
        c = c + t * t
    assert np.cumsum(c)[-1:].view(np.uint64)[0] == np.array([d2], np.float64).view(np.uint64)[0]
    return path


def align_pair(x, y, window=-1, form="scalar"):
    """One unpadded pair -> (D(end) before the sqrt, ascending path)."""
    if form == "scalar":
        D = table_scalar(x, y, window)
        return np.float64(D[-1][-1]), backtrace_scalar(D)
    D, _ = table_wavefront(x, y, window)
    return np.float64(D[-1, -1]), backtrace_wavefront(D)


def align(a, la, b, lb, group_start, members, window=-1, form="scalar"):
    """dsp_dtw_align on padded inputs -> (dist [P], lo [P, Ta], hi [P, Ta], d2 [P]); d2 is D(end)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    P, Ta = len(members), a.shape[1]
    dist, d2 = np.full(P, INF), np.full(P, INF)
    lo, hi = np.full((P, Ta), -1, np.int32), np.full((P, Ta), -1, np.int32)
    for c in range(len(group_start) - 1):
        for p in range(group_start[c], group_start[c + 1]):
            r = int(members[p])
            if not (0 <= r < len(b)) or not (1 <= la[c] <= Ta) or not (1 <= lb[r] <= b.shape[1]):
                continue
            d2[p], path = align_pair(a[c, :la[c]], b[r, :lb[r]], window, form)
            dist[p] = np.float64(math.sqrt(d2[p]))
            lo[p], hi[p] = ranges(path, Ta)
    return dist, lo, hi, d2


def dba_update(tmpl, len_t, seqs, len_s, group_start, members, window=-1, form="scalar"):
    """One DBA update exactly as the header defines it -> (tmpl_out [C, Tt, F], inertia [C])."""
    tmpl, seqs = np.asarray(tmpl, np.float64), np.asarray(seqs, np.float64)
    C, Tt, F = tmpl.shape
    _, lo, hi, d2 = align(tmpl, len_t, seqs, len_s, group_start, members, window, form)
    out, inertia = tmpl.copy(), np.zeros(C)
    for c in range(C):
        L = int(len_t[c])
        valid = [p for p in range(group_start[c], group_start[c + 1]) if lo[p, 0] >= 0]
        if not (1 <= L <= Tt) or not valid:
            continue
        acc, cnt, inert = None, np.zeros(L, np.int64), None
        for p in valid:
            s = seqs[members[p]]
            S = np.empty((L, F))
            for i in range(L):
                row = s[lo[p, i]].copy()
                for j in range(lo[p, i] + 1, hi[p, i] + 1):
                    row = row + s[j]
                S[i] = row
            acc = S if acc is None else acc + S
            cnt += hi[p, :L] - lo[p, :L] + 1
            inert = d2[p] if inert is None else inert + d2[p]
        out[c] = 0.0
        out[c, :L] = acc / cnt[:, None].astype(np.float64)
        inertia[c] = inert
    return out, inertia


def medoid(X, n, members, candidates=256, window=-1):
    """The medoid start: the index (into X) of the candidate -- the class's first min(M, candidates)
    members -- with the smallest sequential sum of squared DTW distances to all M members; ties to the
    earliest."""
    members = np.asarray(members)
    cand = members[:candidates]
    d = R.dtw_pairwise(X[cand], n[cand], X[members], n[members], window)
    return int(cand[int(np.argmin(np.cumsum(d * d, axis=1)[:, -1]))])


def template_fit(X, n, codes, n_iter, window=-1, candidates=256, form="wavefront"):
    """TemplateClassifier.fit on scaled padded sequences -> (templates, lengths, inertia [n_iter, C])."""
    C = int(codes.max()) + 1
    order = np.argsort(codes, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=C))])
    med = [medoid(X, n, order[start[c]:start[c + 1]], candidates, window) for c in range(C)]
    tmpl, len_t = X[med].copy(), n[med].astype(np.int32)
    inertia = np.zeros((n_iter, C))
    for t in range(n_iter):
        tmpl, inertia[t] = dba_update(tmpl, len_t, X, n, start, order, window, form)
    return tmpl, len_t, inertia
