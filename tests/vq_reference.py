"""The numpy restatement of csrc/vq.hip (include/dsp_audiorec.h: dsp_vq_score, dsp_vq_assign,
dsp_vq_accumulate) and of the LBG training around it, in two independent forms that tests/test_vq_host.py
holds against each other bit for bit (a plain helper module like tests/hmm_reference.py: no test, no
fixture):
  form one  ``*_loop``: a per-frame, per-codeword Python loop of explicit np.float64 operations
  form two  vectorised over sequences and codewords (the one the GPU tests compare with: it is fast)
Every operation is one rounded fp64 operation in the order the header gives; sums that have an order
are cumsum (sequential), never np.sum (pairwise)."""
import numpy as np

INF = np.float64(np.inf)


def _valid_k(K, Kmax):
    return 1 <= int(K) <= Kmax


# ---- form one: explicit loops ----
def frame_loop(q, xf):
    """(best, code) of one frame xf [F] among the codewords q [K, F]."""
    best, code = None, 0
    for k in range(len(q)):
        e = np.float64(xf[0]) - np.float64(q[k, 0])
        d = e * e
        for f in range(1, len(xf)):
            e = np.float64(xf[f]) - np.float64(q[k, f])
            d = d + e * e
        if k == 0 or d < best:
            best, code = d, k
    return best, code


def sequence_loop(q, xs, T):
    """(D, code [T]) of the frames xs [n, F] under the codewords q [K, F]."""
    code = np.full(T, -1, np.int32)
    D = None
    for t in range(len(xs)):
        best, code[t] = frame_loop(q, xs[t])
        D = best if t == 0 else D + best
    return D, code


def assign_loop(cb, n_codes, x, n, start, members):
    N, T, _ = x.shape
    Kmax = cb.shape[1]
    dist, code = np.full(len(members), INF), np.full((len(members), T), -1, np.int32)
    with np.errstate(over="ignore"):
        for c in range(len(start) - 1):
            for p in range(start[c], start[c + 1]):
                m = int(members[p])
                if not (_valid_k(n_codes[c], Kmax) and 0 <= m < N and 1 <= n[m] <= T):
                    continue
                dist[p], code[p] = sequence_loop(cb[c, :n_codes[c]], x[m, :n[m]], T)
    return dist, code


def label_of(score):
    label = np.full(len(score), -1, np.int32)
    for r in range(len(score)):
        best = INF
        for c in range(score.shape[1]):
            if score[r, c] < best:
                best, label[r] = score[r, c], c
    return label


def score_loop(cb, n_codes, x, n):
    N, C = len(x), len(cb)
    start = np.arange(C + 1) * N
    dist, _ = assign_loop(cb, n_codes, x, n, start, np.tile(np.arange(N), C))
    score = dist.reshape(C, N).T.copy()
    return score, label_of(score)


def member_valid(K, Kmax, m, N, n, T, code_row):
    if not (_valid_k(K, Kmax) and 0 <= m < N and 1 <= n[m] <= T):
        return False
    c = code_row[:n[m]]
    return bool(((c >= 0) & (c < K)).all())


def accumulate_loop(cb_prev, n_codes, x, n, start, members, code, dist):
    C, Kmax, F = cb_prev.shape
    N, T, _ = x.shape
    centroid, cnt = np.zeros((C, Kmax, F)), np.zeros((C, Kmax), np.int32)
    n_valid, total = np.zeros(C, np.int32), np.zeros(C)
    for c in range(C):
        K = int(n_codes[c])
        acc, seen, tot = np.zeros((Kmax, F)), np.zeros(Kmax, bool), None
        for p in range(start[c], start[c + 1]):
            m = int(members[p])
            if not member_valid(K, Kmax, m, N, n, T, code[p]):
                continue
            X, got = np.zeros((Kmax, F)), np.zeros(Kmax, np.int64)
            for t in range(n[m]):
                j = code[p, t]
                for f in range(F):
                    X[j, f] = x[m, t, f] if got[j] == 0 else X[j, f] + x[m, t, f]
                got[j] += 1
            for j in range(K):
                if got[j] == 0:
                    continue
                for f in range(F):
                    acc[j, f] = X[j, f] if not seen[j] else acc[j, f] + X[j, f]
                seen[j] = True
                cnt[c, j] += got[j]
            tot = np.float64(dist[p]) if tot is None else tot + np.float64(dist[p])
            n_valid[c] += 1
        if n_valid[c] == 0:
            centroid[c], cnt[c] = cb_prev[c], 0
            continue
        total[c] = tot
        for j in range(K):
            centroid[c, j] = acc[j] / np.float64(cnt[c, j]) if cnt[c, j] > 0 else cb_prev[c, j]
    return centroid, cnt, n_valid, total


# ---- form two: vectorised ----
def nearest(q, x):
    """(best [...], code [...]) of the frames x [..., F] among the codewords q [K, F]."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = x[..., None, 0] - q[:, 0]
        d = e * e
        for f in range(1, x.shape[-1]):
            e = x[..., None, f] - q[:, f]
            d = d + e * e
    code = np.argmin(d, axis=-1)  # the first of the smallest
    return np.take_along_axis(d, code[..., None], axis=-1)[..., 0], code.astype(np.int32)


def _rows(cb, n_codes, c, x, n, rows):
    """(D [len(rows)], code [len(rows), T]) of the sequences ``rows`` (any integers) under codebook c."""
    N, T, _ = x.shape
    rows = np.asarray(rows, np.int64)
    D, code = np.full(len(rows), INF), np.full((len(rows), T), -1, np.int32)
    ok = (rows >= 0) & (rows < N)
    ok[ok] = (n[rows[ok]] >= 1) & (n[rows[ok]] <= T)
    if not _valid_k(n_codes[c], cb.shape[1]) or not ok.any():
        return D, code
    r = rows[ok]
    best, cd = nearest(cb[c, :n_codes[c]], x[r])
    live = np.arange(T)[None, :] < n[r][:, None]
    with np.errstate(invalid="ignore"):
        run = np.cumsum(np.where(live, best, 0.0), axis=1)  # sequential: D = best(0) + best(1) + ...
    D[ok] = run[np.arange(len(r)), n[r] - 1]
    code[ok] = np.where(live, cd, -1)
    return D, code


def score(cb, n_codes, x, n):
    """dsp_vq_score: (score float64 [N, C], label int32 [N])."""
    n = np.asarray(n)
    if not len(cb):
        return np.zeros((len(x), 0)), np.full(len(x), -1, np.int32)
    out = np.stack([_rows(cb, n_codes, c, x, n, np.arange(len(x)))[0] for c in range(len(cb))], axis=1)
    return out, np.where(np.isinf(out).all(axis=1), -1, np.argmin(out, axis=1)).astype(np.int32)


def assign(cb, n_codes, x, n, start, members):
    """dsp_vq_assign: (dist float64 [P], code int32 [P, T])."""
    n, members = np.asarray(n), np.asarray(members)
    dist, code = np.full(len(members), INF), np.full((len(members), x.shape[1]), -1, np.int32)
    for c in range(len(start) - 1):
        if start[c + 1] > start[c]:
            dist[start[c]:start[c + 1]], code[start[c]:start[c + 1]] = _rows(cb, n_codes, c, x, n, members[start[c]:start[c + 1]])
    return dist, code


def _ordered_sums(keys, vals):
    """The values vals [M, F] of each key added in the order they stand (the first is the value itself):
    (the keys ascending, their sums, their counts).  Step i adds the i-th value of every key that has one."""
    order = np.argsort(keys, kind="stable")
    k, v = keys[order], vals[order]
    uniq, first, counts = np.unique(k, return_index=True, return_counts=True)
    acc = v[first].copy()
    for i in range(1, int(counts.max())):
        more = counts > i
        acc[more] = acc[more] + v[first[more] + i]
    return uniq, acc, counts


def accumulate(cb_prev, n_codes, x, n, start, members, code, dist):
    """dsp_vq_accumulate: (centroid float64 [C, Kmax, F], cnt int32 [C, Kmax], n_valid int32 [C], total
    float64 [C]).  All (member, cell) sums of a codebook advance together one frame at a time, then all
    cell sums one member at a time (``_ordered_sums``)."""
    C, Kmax, F = cb_prev.shape
    N, T, _ = x.shape
    n, members, code = np.asarray(n), np.asarray(members), np.asarray(code)
    centroid, cnt = np.zeros((C, Kmax, F)), np.zeros((C, Kmax), np.int32)
    n_valid, total = np.zeros(C, np.int32), np.zeros(C)
    for c in range(C):
        K = int(n_codes[c])
        ps = np.array([p for p in range(start[c], start[c + 1])
                       if member_valid(K, Kmax, int(members[p]), N, n, T, code[p])], np.int64)
        n_valid[c] = len(ps)
        if not len(ps):
            centroid[c] = cb_prev[c]
            continue
        total[c] = np.cumsum(np.asarray(dist, np.float64)[ps])[-1]
        mem = members[ps]
        live = np.arange(T)[None, :] < n[mem][:, None]  # [members, T], row-major: list order, then t ascending
        rank = np.broadcast_to(np.arange(len(ps))[:, None], live.shape)[live]
        key, X, m = _ordered_sums(rank * Kmax + code[ps][live], x[mem][live])
        cell, acc, _ = _ordered_sums(key % Kmax, X)  # key ascending: within a cell the members in list order
        np.add.at(cnt[c], key % Kmax, m.astype(np.int32))
        centroid[c, :K] = cb_prev[c, :K]
        centroid[c, cell] = acc / cnt[c, cell].astype(np.float64)[:, None]
    return centroid, cnt, n_valid, total


# ---- the numpy pieces of LBG training ----
def split(cb, eps):
    """Codeword j becomes 2 j = c + eps and 2 j + 1 = c - eps."""
    eps = np.float64(eps)
    return np.stack([cb + eps, cb - eps], axis=-2).reshape(cb.shape[:-2] + (2 * cb.shape[-2], cb.shape[-1]))


def repair_empty(cb, cnt, n_codes, eps):
    """Each empty cell j ascending takes half of the fullest cell (cnt >= 2, ties to the smaller index)."""
    cb, cnt, eps = cb.copy(), np.asarray(cnt).astype(np.int64).copy(), np.float64(eps)
    for c in range(len(cb)):
        for j in range(int(n_codes[c])):
            if cnt[c, j] > 0:
                continue
            donor, most = -1, 1
            for i in range(int(n_codes[c])):
                if cnt[c, i] > most:
                    donor, most = i, cnt[c, i]
            if donor < 0:
                continue
            cb[c, j], cb[c, donor] = cb[c, donor] + eps, cb[c, donor] - eps
            cnt[c, j] = most // 2
            cnt[c, donor] = most - most // 2
    return cb, cnt


def fit(X, n, codes, n_codes, n_iter=10, eps=0.01):
    """VqClassifier.fit on the normalised padded sequences X [N, T, F] with class codes 0 .. C-1:
    (codebooks [C, K, F], counts [C, K], totals [rounds, C], repairs: how many cells a repair moved)."""
    n, codes = np.asarray(n), np.asarray(codes)
    C, F = int(codes.max()) + 1, X.shape[2]
    order = np.argsort(codes, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=C))])
    K, sizes = 1, np.ones(C, np.int32)
    cb, cnt, _, _ = accumulate(np.zeros((C, 1, F)), sizes, X, n, start, order, np.zeros((len(order), X.shape[1]), np.int32),
                               np.zeros(len(order)))
    totals, repairs = [], 0
    while K < n_codes:
        cb, K = split(cb, eps), 2 * K
        sizes = np.full(C, K, np.int32)
        code = None
        for _ in range(n_iter):
            dist, new_code = assign(cb, sizes, X, n, start, order)
            cen, cnt, _, total = accumulate(cb, sizes, X, n, start, order, new_code, dist)
            totals.append(total)
            cb, moved = repair_empty(cen, cnt, sizes, eps)
            repairs += int(((cnt == 0) & (moved > 0)).sum())
            same = code is not None and np.array_equal(new_code, code)
            code = new_code
            if same:
                break
    return cb, cnt.astype(np.int64), np.array(totals, np.float64).reshape(len(totals), C), repairs
