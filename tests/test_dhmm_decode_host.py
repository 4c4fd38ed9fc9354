"""CPU tests of the connected-word decoding definition (tests/dhmm_decode_reference.py) and of the host side
on it: the two forms of the restatement agree bit for bit, the result is the brute force's over all word
sequences and state paths with the walk-back tie order, the consequences of the definition against the
isolated-word Viterbi of tests/dhmm_reference.py, the word error rate, and the loaded library's argument
checks."""
import ctypes

import numpy as np
import pytest

import dhmm_decode_reference as R
import dhmm_reference as D

INF = np.inf


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def same(got, want):
    for g, w, name in zip(got, want, ("score", "n_words", "words", "start", "cum")):
        g, w = (bits(v) if v.dtype == np.float64 else v for v in (g, w))
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


def random_corpus():
    """Seven models (one with n_states 0, one with Smax + 1) over K = 9 symbols with a +inf emission, an
    all-+inf emission row, a +inf stay and +inf entry costs; 40 utterances of up to 30 frames, three with a
    symbol outside the alphabet, two with a bad length."""
    model = D.random_models(np.array([3, 1, 0, 5, 2, 6, 4], np.int32), 5, 9, seed=5)
    model.emit[0, 1, 3] = model.emit[3, 2, :] = model.stay[4, 0] = INF
    enter = np.array([0.5, 2.0, 0.0, INF, 0.0, 1.0, 0.25])
    sym, n = D.random_symbols(40, 30, 9, seed=6)
    sym[3, 0], sym[4, n[4] - 1], sym[5, n[5] // 2] = 9, -1, 2 ** 31 - 1
    n[[7, 8]] = [0, 31]
    return model, enter, sym, n


def test_the_two_forms_agree():
    model, enter, sym, n = random_corpus()
    table = R.decode(model, sym, n, enter, form="table")
    same(R.decode(model, sym, n, enter, form="rows"), table)
    score, n_words, words, start, cum = table
    assert np.isinf(score[[3, 4, 5, 7, 8]]).all() and (n_words[[3, 4, 5, 7, 8]] == 0).all()
    assert np.isfinite(score).sum() >= 30 and n_words.max() >= 3 and not np.isnan(score).any()
    assert not np.isin(words, [2, 3, 5]).any()  # n_states 0, enter +inf, n_states Smax + 1
    for i in np.flatnonzero(n_words):
        k = n_words[i]
        assert start[i, 0] == 0 and (np.diff(start[i, :k]) > 0).all() and (words[i, k:] == -1).all()
        assert bits(cum[i, k - 1]) == bits(score[i]) and np.isinf(cum[i, k:]).all()
    same(R.decode(model, sym, n, None, form="rows"), R.decode(model, sym, n, np.zeros(7), form="table"))


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_the_two_forms_agree_on_the_tie_corpus(seed):
    """Conditions on the input as well: at least 8 % of the decided cells have a == b and at least 10 % of
    the frames have their exit minimum in two or more models."""
    model, enter, sym, n = R.tie_corpus(seed)
    stats = [0, 0, 0, 0]
    rows = R.decode(model, sym, n, enter, form="rows", stats=stats)
    print("cells %d tied %.3f, frames %d shared %.3f" % (stats[0], stats[1] / stats[0], stats[2], stats[3] / stats[2]))
    assert stats[0] > 20000 and stats[1] / stats[0] >= 0.08, stats
    assert stats[2] > 500 and stats[3] / stats[2] >= 0.10, stats
    same(rows, R.decode(model, sym, n, enter, form="table"))
    assert np.isfinite(rows[0]).all() and rows[1].min() >= 1 and rows[1].max() >= 3


def brute_force(row, model, cost):
    """(cost, words, starts) over every word sequence and state path, each path costed in the recurrence's
    own association e + (prev + trans).  Among the paths of the smallest cost the walk-back order decides:
    compared from the last frame backwards, the smaller last model, then at every frame staying before
    having advanced or entered, and at a boundary the smaller model before it."""
    n, C = len(row), len(model.n_states)
    ms = [model.one(c) for c in range(C)]
    best = [None]

    def step(t, c, s, prev, key, words):
        if t == n:
            if s == len(ms[c][1]) - 1 and prev < INF:
                full = (prev, (c,) + key)
                if best[0] is None or full < best[0][:2]:
                    best[0] = (prev, (c,) + key, list(words))
            return
        for c2 in range(C):  # frame t in state (c2, s2)
            if ms[c2] is None:
                continue
            emit, stay, adv = ms[c2]
            opts = []
            if t > 0 and c2 == c:
                opts.append((s, stay[s], (0,), False))
                if s + 1 < len(stay):
                    opts.append((s + 1, adv[s], (1, -1), False))
            if t == 0 or s == len(ms[c][1]) - 1:
                opts.append((0, cost[c2], (1, c if t else -1), True))
            for s2, trans, kind, new in opts:
                v = np.float64(emit[s2, row[t]]) + (prev + np.float64(trans))
                if not v < INF:  # never a minimum
                    continue
                step(t + 1, c2, s2, v, (kind,) + key, words + [(c2, t)] if new else words)

    c0 = next(c for c in range(C) if ms[c] is not None)
    step(0, c0, 0, np.float64(0.0), (), [])
    if best[0] is None:
        return INF, [], []
    return best[0][0], [w for w, _ in best[0][2]], [b for _, b in best[0][2]]


@pytest.mark.parametrize("corpus", ("dyadic", "random"))
def test_the_result_is_the_brute_force_minimum(corpus):
    rng = np.random.default_rng(31 if corpus == "dyadic" else 32)
    several = tied = 0
    for case in range(100):
        C, Smax, K = int(rng.integers(1, 4)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
        states = rng.integers(1, Smax + 1, C).astype(np.int32)
        if corpus == "dyadic":
            model = D.Model(rng.integers(0, 4, (C, Smax, K)) / 2.0, rng.integers(0, 3, (C, Smax)) / 2.0,
                            rng.integers(0, 3, (C, Smax)) / 2.0, states)
            enter = rng.integers(0, 4, C) / 2.0
        else:
            model, enter = D.random_models(states, Smax, K, seed=100 + case), rng.uniform(0, 2, C)
        if case % 7 == 0:
            enter[rng.integers(0, C)] = INF
        n = int(rng.integers(1, 8)) if C * Smax < 9 else int(rng.integers(1, 7))
        row = [int(k) for k in rng.integers(0, K, n)]
        want = brute_force(row, model, R.enter_of(model, enter))
        for form in ("table", "rows"):
            score, found = R.decode_one(row, model, R.enter_of(model, enter), form)
            assert bits(score) == bits(want[0]), (case, form)
            assert [w for w, _, _ in found] == want[1] and [b for _, b, _ in found] == want[2], (case, form, found, want)
        several += len(want[1]) > 1
        tied += np.isfinite(want[0])
    print(corpus, several, tied)
    assert several >= 15 and tied >= 60


def test_a_single_word_is_the_isolated_score():
    """enter = 0.0 and n < 2 min S: only one word fits, so the score is the smallest dsp_dhmm_score bit for bit
    and words[0] its label."""
    model = D.random_models(np.array([4, 5, 4, 6], np.int32), 6, 11, seed=41)
    sym, n = D.random_symbols(30, 7, 11, seed=42, lo=1)
    score, n_words, words, start, cum = R.decode(model, sym, n, np.zeros(4))
    iso = np.stack([[D.viterbi_table(sym[i, :n[i]], *model.one(c))[0] for c in range(4)] for i in range(30)])
    assert np.array_equal(bits(score), bits(iso.min(axis=1))) and np.isfinite(score).sum() >= 10
    assert np.array_equal(n_words, np.isfinite(score)) and np.array_equal(words[:, 0], D.label_of(iso))
    assert (start[np.isfinite(score), 0] == 0).all() and np.isinf(score[n < 4]).all()


def test_the_first_word_is_the_isolated_score_of_its_prefix():
    """enter[words[0]] = 0.0: cum[0] is dsp_dhmm_score of sym[0 : start[1]] under model words[0]."""
    model = D.random_models(np.array([2, 3, 1, 4], np.int32), 4, 6, seed=43)
    sym, n = D.random_symbols(30, 25, 6, seed=44, lo=8)
    score, n_words, words, start, cum = R.decode(model, sym, n, np.zeros(4))
    assert (n_words >= 2).sum() >= 20
    for i in np.flatnonzero(n_words >= 2):
        got = D.viterbi_table(sym[i, :start[i, 1]], *model.one(words[i, 0]))[0]
        assert bits(got) == bits(cum[i, 0]), i


def test_a_duplicated_model_never_appears():
    model = D.random_models(np.array([2, 3, 2, 3, 1], np.int32), 3, 6, seed=45)
    for a in (model.emit, model.stay, model.adv):
        a[2], a[3] = a[0], a[1]
    sym, n = D.random_symbols(30, 25, 6, seed=46, lo=5)
    enter = np.array([0.5, 0.25, 0.5, 0.25, 1.0])
    score, n_words, words, start, cum = R.decode(model, sym, n, enter)
    assert np.isin(words, [0, 1]).sum() > 40 and not np.isin(words, [2, 3]).any()


def test_max_words_truncation():
    model, enter = D.random_models(np.array([1, 2, 1, 3], np.int32), 3, 6, seed=47), np.array([0.5, 0.0, 1.0, 0.0])
    sym, n = D.random_symbols(12, 20, 6, seed=48, lo=10)
    full = R.decode(model, sym, n, enter)
    assert full[2].shape == (12, 20) and full[1].min() >= 3
    for mw in (1, 2, int(full[1].max()) - 1, int(full[1].max())):
        score, n_words, words, start, cum = R.decode(model, sym, n, enter, max_words=mw)
        assert np.array_equal(bits(score), bits(full[0])) and np.array_equal(n_words, full[1])
        assert words.shape == (12, mw) and np.array_equal(words, full[2][:, :mw]) and np.array_equal(start, full[3][:, :mw])
        assert np.array_equal(bits(cum), bits(full[4][:, :mw]))


def test_word_error_rate():
    from src.models import word_error_rate
    assert word_error_rate([[1, 2, 3]], [[1, 2, 3]]) == 0.0
    assert word_error_rate([[1, 2, 3]], [[1, 3]]) == 1 / 3          # a deletion
    assert word_error_rate([[1, 2, 3]], [[1, 2, 4, 3]]) == 1 / 3    # an insertion
    assert word_error_rate([[1, 2, 3]], [[1, 5, 3]]) == 1 / 3       # a substitution
    assert word_error_rate([[1, 2, 3]], [[]]) == 1.0 and word_error_rate([[1]], [[2, 3, 4]]) == 3.0
    assert word_error_rate([["a", "b"], ["c", "d", "e", "f"]], [["b"], ["c", "x", "e", "f", "g"]]) == 3 / 6
    assert word_error_rate([np.array([7, 7, 8]), []], [np.array([7, 8]), [1]]) == 2 / 3
    with pytest.raises(ValueError):
        word_error_rate([[1]], [[1], [2]])
    with pytest.raises(ValueError):
        word_error_rate([[]], [[1]])


def test_decode_surface_without_a_device():
    from src.models import DiscreteHmmClassifier
    from src.pipeline import DHMM_DECODE_MAX_MODELS, dhmm_decode
    assert DHMM_DECODE_MAX_MODELS == R.MAX_MODELS == 64
    assert callable(dhmm_decode) and callable(DiscreteHmmClassifier.decode)


def test_abi_argument_checks():
    """The plan's bounds and the NULL checks, answered on the host before any launch."""
    from src import _hip
    lib = _hip.load_library()
    wb = lib.dsp_dhmm_decode_workspace_bytes
    assert wb(64, 100, 1024, 32, 256) >= 256 * 32 * 64 * 8 and wb(1, 0, 1, 1, 1) > 0
    assert wb(10, 5, 64, 8, 64) < wb(10, 5, 64, 9, 64) < wb(10, 5, 64, 17, 64) and wb(10, 5, 64, 5, 64) == wb(64, 9, 9, 8, 64)
    for args in ((65, 4, 64, 5, 64), (0, 4, 64, 5, 64), (-1, 4, 64, 5, 64), (3, 4, 1025, 5, 64), (3, 4, 0, 5, 64),
                 (3, 4, 64, 5, 257), (3, 4, 64, 5, 0), (3, 4, 64, 33, 64), (3, 4, 64, 0, 64), (3, -1, 64, 5, 64)):
        assert wb(*args) == 0, args
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30

    def call(C=3, Smax=5, K=64, N=4, T=64, max_words=4, emit=p, sym=p, outs=(p, p, p, p, p), ws=p, nws=big):
        return lib.dsp_dhmm_decode(emit, p, p, p, None, C, Smax, K, sym, p, N, T, max_words, *outs, ws, nws, None)

    for bad in (dict(C=65), dict(C=0), dict(T=1025), dict(T=0), dict(K=257), dict(K=0), dict(Smax=33), dict(Smax=0),
                dict(max_words=0), dict(max_words=65), dict(N=-1), dict(emit=None), dict(sym=None)):
        assert call(**bad) == _hip.DSP_ERR_ARGS, bad
    assert call(ws=None, nws=0) == _hip.DSP_ERR_WORKSPACE and call(nws=wb(3, 4, 64, 5, 64) - 1) == _hip.DSP_ERR_WORKSPACE
    assert call(N=0, ws=None, nws=0) == _hip.DSP_OK
    assert call(outs=(None,) * 5, ws=None, nws=0) == _hip.DSP_OK
    assert call(N=0, C=65) == _hip.DSP_ERR_ARGS  # the bounds come before "nothing to do"
