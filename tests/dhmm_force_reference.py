"""numpy restatement of csrc/dhmm_force.hip (include/dsp_audiorec.h: dsp_dhmm_force_align,
dsp_dhmm_force_accumulate) and of the host side on it (dhmm_flat_segmentation,
DiscreteHmmClassifier.fit_connected); a plain helper module like tests/dhmm_decode_reference.py: no test, no
fixture.

Every value is defined bit for bit -- fp64 add and compare in a fixed order, integer counts -- so everything
here is compared with array_equal on raw bits.  The forced pass exists in two independent forms:
  "table"  the definition's per-cell loop over the chain of concatenated states: V and a back-pointer of every
           (frame, chain state) stored, the path walked back over the back-pointers;
  "rows"   all positions and states of a frame advance together as [Wmax, Smax] arrays; one direction bit per
           cell, and the walk follows (position, state) through the bits.
"""
import numpy as np

import dhmm_decode_reference as R
import dhmm_reference as D

INF = np.float64(np.inf)
MAX_WORDS = 64


def transcript_of(model, trans_row, L, Wmax):
    """The transcript's L model indices, or None where the result is forced: L outside 1 .. Wmax, an index
    outside [0, C), a model whose n_states is outside 1 .. Smax."""
    L = int(L)
    if L < 1 or L > Wmax:
        return None
    C, Smax = model.emit.shape[:2]
    words = [int(w) for w in trans_row[:L]]
    for w in words:
        if w < 0 or w >= C or not 1 <= int(model.n_states[w]) <= Smax:
            return None
    return words


def force_table(row, model, cost, words):
    """(score, seg as a list of per-position lists, or None when the score is +inf) by the per-cell loop."""
    n = len(row)
    chain = [(i, s) for i, w in enumerate(words) for s in range(int(model.n_states[w]))]
    J = len(chain)
    prev = np.full(J, INF)
    back = np.zeros((n, J), bool)
    for t in range(n):
        cur = np.full(J, INF)
        for j, (i, s) in enumerate(chain):
            w = words[i]
            e = np.float64(model.emit[w, s, row[t]])
            a = prev[j] + np.float64(model.stay[w, s])
            if s > 0:
                b = prev[j - 1] + np.float64(model.adv[w, s - 1])
            elif i > 0:
                b = prev[j - 1] + np.float64(cost[w])
            elif t == 0:
                b = np.float64(0.0) + np.float64(cost[w])
            else:
                b = INF
            if b < a:
                cur[j], back[t, j] = e + b, True
            else:
                cur[j] = e + a
        prev = cur
    score = prev[J - 1]
    if not score < INF:
        return INF, None
    first, j = [0] * J, J - 1
    for t in range(n - 1, -1, -1):
        if back[t, j]:
            first[j] = t
            j -= 1
            if j < 0:
                break
    assert j < 0 and first[0] == 0
    seg = [[] for _ in words]
    for (i, s), f in zip(chain, first):
        seg[i].append(f)
    return score, seg


def force_rows(row, model, cost, words, Wmax, stats=None):
    """The same with every position and state of a frame in one array operation.  stats: a two-entry list
    that collects [decided cells, of them a == b] -- a decided cell is one of a chain state whose min(a, b)
    is finite."""
    n, L = len(row), len(words)
    Smax = model.emit.shape[1]
    w = np.array(words, np.int64)
    S = np.zeros(Wmax, np.int64)
    S[:L] = model.n_states[w]
    valid = np.arange(Smax)[None, :] < S[:, None]
    wp = np.zeros(Wmax, np.int64)
    wp[:L] = w
    emit = np.where(valid[:, :, None], model.emit[wp], INF)  # [Wmax, Smax, K]
    stay, adv = np.where(valid, model.stay[wp], 0.0), np.where(valid, model.adv[wp], 0.0)
    enter = np.where(np.arange(Wmax) < L, np.asarray(cost, np.float64)[wp], INF)
    last = np.maximum(S - 1, 0)
    V = np.full((Wmax, Smax), INF)
    bits = np.zeros((n, Wmax, Smax), bool)
    for t in range(n):
        ex = V[np.arange(Wmax), last]
        come = np.concatenate([[np.float64(0.0) if t == 0 else INF], ex[:-1]])
        a = V + stay
        b = np.concatenate([(come + enter)[:, None], V[:, :-1] + adv[:, :-1]], axis=1)
        bits[t] = (b < a) & valid
        if stats is not None:
            cell = valid & (np.minimum(a, b) < INF)
            stats[0] += int(cell.sum())
            stats[1] += int((cell & (a == b)).sum())
        V = np.where(valid, emit[:, :, row[t]] + np.where(b < a, b, a), INF)
    score = V[L - 1, S[L - 1] - 1]
    if not score < INF:
        return INF, None
    seg = [[0] * int(S[i]) for i in range(L)]
    i, s = L - 1, int(S[L - 1]) - 1
    for t in range(n - 1, -1, -1):
        if not bits[t, i, s]:
            continue
        seg[i][s] = t
        if s > 0:
            s -= 1
        else:
            i -= 1
            if i < 0:
                break
            s = int(S[i]) - 1
    assert i < 0
    return score, seg


def align(model, sym, n, trans, n_trans, enter=None, form="rows", stats=None):
    """dsp_dhmm_force_align: (score float64 [N], seg int32 [N, Wmax, Smax])."""
    N, T = sym.shape
    Wmax = trans.shape[1]
    Smax, K = model.emit.shape[1:]
    cost = R.enter_of(model, enter)
    score, seg = np.full(N, INF), np.full((N, Wmax, Smax), -1, np.int32)
    for u in range(N):
        row = R._clean(sym[u], n[u], T, K)
        words = transcript_of(model, trans[u], n_trans[u], Wmax)
        if row is None or words is None:
            continue
        if form == "table":
            sc, sg = force_table(row, model, cost, words)
        else:
            sc, sg = force_rows(row, model, cost, words, Wmax, stats)
        score[u] = sc
        if sg is not None:
            for i, firsts in enumerate(sg):
                seg[u, i, :len(firsts)] = firsts
    return score, seg


def brute_force(row, model, cost, words):
    """The smallest cost over ALL monotone state paths of the chain, each costed left to right as
    e + (prev + trans): (score, set of the first-frame tuples of the paths that reach it)."""
    n = len(row)
    chain = [(words[i], s, i) for i in range(len(words)) for s in range(int(model.n_states[words[i]]))]
    J = len(chain)
    best, arg = INF, set()
    if n < J:
        return best, arg

    def cuts(j, lo):  # first frames of chain states j .. J-1, strictly increasing, each > lo
        if j == J:
            yield ()
            return
        for f in range(lo + 1, n - (J - 1 - j)):
            for rest in cuts(j + 1, f):
                yield (f,) + rest

    for tail in cuts(1, 0):
        first = (0,) + tail
        j, v = 0, None
        for t in range(n):
            moved = j + 1 < J and first[j + 1] == t
            if moved:
                j += 1
            w, s, i = chain[j]
            e = np.float64(model.emit[w, s, row[t]])
            if t == 0:
                v = e + (np.float64(0.0) + np.float64(cost[w]))
            elif moved:
                v = e + (v + (np.float64(model.adv[w, s - 1]) if s > 0 else np.float64(cost[w])))
            else:
                v = e + (v + np.float64(model.stay[w, s]))
        if v < best:
            best, arg = v, {first}
        elif v == best and v < INF:
            arg.add(first)
    return best, arg


def flat_segmentation(lengths, trans, n_trans, n_states, Smax):
    """pipeline.dhmm_flat_segmentation: concatenated state j of J = sum S_i begins at frame floor(j n / J);
    -1 everywhere when n < J or the transcript is invalid."""
    N, Wmax = trans.shape
    C = len(n_states)
    seg = np.full((N, Wmax, Smax), -1, np.int32)
    for u in range(N):
        L, n = int(n_trans[u]), int(lengths[u])
        if L < 1 or L > Wmax:
            continue
        words = [int(w) for w in trans[u, :L]]
        if any(w < 0 or w >= C or not 1 <= int(n_states[w]) <= Smax for w in words):
            continue
        J = sum(int(n_states[w]) for w in words)
        if n < J:
            continue
        j = 0
        for i, w in enumerate(words):
            for s in range(int(n_states[w])):
                seg[u, i, s] = (j * n) // J
                j += 1
    return seg


def accumulate(n_states, K, sym, n, trans, n_trans, seg):
    """dsp_dhmm_force_accumulate by a per-frame loop: (cnt_emit int32 [C, Smax, K], cnt int32 [C, Smax],
    n_valid int32 [C], valid int32 [N])."""
    N, T = sym.shape
    Wmax, Smax = seg.shape[1:]
    C = len(n_states)
    cnt_emit, cnt = np.zeros((C, Smax, K), np.int32), np.zeros((C, Smax), np.int32)
    n_valid, valid = np.zeros(C, np.int32), np.zeros(N, np.int32)
    for u in range(N):
        L, nu = int(n_trans[u]), int(n[u])
        if nu < 1 or nu > T or L < 1 or L > Wmax:
            continue
        words = [int(w) for w in trans[u, :L]]
        if any(w < 0 or w >= C or not 1 <= int(n_states[w]) <= Smax for w in words):
            continue
        row = sym[u, :nu]
        if ((row < 0) | (row >= K)).any():
            continue
        want_pad = np.ones((Wmax, Smax), bool)
        chain, first = [], []
        for i, w in enumerate(words):
            for s in range(int(n_states[w])):
                want_pad[i, s] = False
                chain.append((w, s))
                first.append(int(seg[u, i, s]))
        if (seg[u][want_pad] != -1).any() or first[0] != 0:
            continue
        first.append(nu)
        if any(first[j] >= first[j + 1] for j in range(len(chain))):
            continue
        state_of = np.zeros(nu, np.int64)
        for j in range(len(chain)):
            state_of[first[j]:first[j + 1]] = j
        for t in range(nu):  # the per-frame loop
            w, s = chain[state_of[t]]
            cnt_emit[w, s, row[t]] += 1
            cnt[w, s] += 1
        for w in words:
            n_valid[w] += 1
        valid[u] = 1
    return cnt_emit, cnt, n_valid, valid


def total_of(score, valid):
    """A round's objective: the valid utterances' forced scores added in utterance order, from the first."""
    tot = None
    for v, ok in zip(score, valid):
        if ok:
            tot = np.float64(v) if tot is None else tot + np.float64(v)
    return np.float64(0.0) if tot is None else tot


def fit_connected(sym, n, trans, n_trans, states, K, n_iter=10, alpha=0.5, trans_floor=1e-3, enter=None, form="rows"):
    """DiscreteHmmClassifier.fit_connected from the tokeniser's symbols on: (model, totals [rounds], the last
    seg).  A word without an instance in a valid utterance of the flat start raises ValueError."""
    states = np.asarray(states, np.int32)
    Smax = int(states.max())
    seg = flat_segmentation(n, trans, n_trans, states, Smax)
    st = accumulate(states, K, sym, n, trans, n_trans, seg)
    if (st[2] == 0).any():
        raise ValueError("word %d has no instance" % int(np.argmin(st[2])))
    model = D.build_model(*st[:3], states, alpha, trans_floor)
    totals = []
    for _ in range(n_iter):
        sc, new_seg = align(model, sym, n, trans, n_trans, enter, form)
        st = accumulate(states, K, sym, n, trans, n_trans, new_seg)
        totals.append(total_of(sc, st[3]))
        model = D.build_model(*st[:3], states, alpha, trans_floor, prev=model)
        same = np.array_equal(new_seg, seg)
        seg = new_seg
        if same:
            break
    return model, np.array(totals, np.float64), seg


# ---- test corpora ----
def random_transcripts(N, Wmax, C, seed, lo=1, counts=None):
    """trans int32 [N, Wmax] uniform over the models with word counts in lo .. Wmax (or the given ones); behind
    each count the row holds garbage: -1, C, 2^31 - 1 and INT_MIN in turn."""
    rng = np.random.default_rng(seed)
    L = rng.integers(lo, Wmax + 1, N).astype(np.int32) if counts is None else np.asarray(counts, np.int32)
    trans = rng.integers(0, C, (N, Wmax)).astype(np.int64)
    junk = np.where(D.GARBAGE == 0, C, D.GARBAGE)[(np.arange(Wmax)[None, :] + np.arange(N)[:, None]) % 4]
    behind = np.arange(Wmax)[None, :] >= np.clip(L, 0, Wmax)[:, None]
    return np.where(behind, junk, trans).astype(np.int32), L


def tie_corpus(seed, N=24, Wmax=4):
    """dhmm_decode_reference.tie_corpus' dyadic models and symbols with random transcripts of 1 .. Wmax of its
    ten models: every sum is exact, so many cells tie exactly."""
    model, enter, sym, n = R.tie_corpus(seed, N)
    trans, L = random_transcripts(N, Wmax, 10, seed + 2)
    return model, enter, sym, n, trans, L
