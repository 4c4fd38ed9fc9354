"""CPU tests of connected-word decoding under a word-pair grammar: the definition
(tests/dhmm_grammar_reference.py) and the host side on it.  The two forms of the restatement agree bit for
bit, the result is the brute force's over all word sequences and state paths with the walk-back tie order, four
consequences of the definition against the loop decoder, the forced alignment and the isolated-word Viterbi of
the neighbouring restatements, WordPairGrammar by hand, and the loaded library's argument checks."""
import ctypes

import numpy as np
import pytest

import dhmm_decode_reference as R
import dhmm_force_reference as F
import dhmm_grammar_reference as GR
import dhmm_reference as D

INF = np.inf
NAMES = ("score", "n_words", "words", "start")


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def same(got, want):
    for g, w, name in zip(got, want, NAMES):
        g, w = (bits(v) if v.dtype == np.float64 else v for v in (g, w))
        assert g.shape == w.shape and np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


def random_corpus():
    """test_dhmm_decode_host's corpus -- seven models (one with n_states 0, one with Smax + 1) over K = 9 symbols
    with a +inf emission, an all-+inf emission row and a +inf stay; 40 utterances of up to 30 frames, three with a
    symbol outside the alphabet, two with a bad length -- and a grammar with +inf entries in enter, pair and
    leave; the cost rows and columns of the two invalid models are NaN."""
    model = D.random_models(np.array([3, 1, 0, 5, 2, 6, 4], np.int32), 5, 9, seed=5)
    model.emit[0, 1, 3] = model.emit[3, 2, :] = model.stay[4, 0] = INF
    sym, n = D.random_symbols(40, 30, 9, seed=6)
    sym[3, 0], sym[4, n[4] - 1], sym[5, n[5] // 2] = 9, -1, 2 ** 31 - 1
    n[[7, 8]] = [0, 31]
    enter, pair, leave = GR.random_grammar(7, seed=7, forbid=0.25)
    enter[1], leave[4] = INF, INF
    for a in (enter, leave, pair, pair.T):
        a[[2, 5]] = np.nan
    return model, sym, n, enter, pair, leave


def test_the_two_forms_agree():
    model, sym, n, enter, pair, leave = random_corpus()
    table = GR.decode(model, sym, n, enter, pair, leave, form="table")
    same(GR.decode(model, sym, n, enter, pair, leave, form="rows"), table)
    score, n_words, words, start = table
    assert np.isinf(score[[3, 4, 5, 7, 8]]).all() and (n_words[[3, 4, 5, 7, 8]] == 0).all()
    assert np.isfinite(score).sum() >= 25 and n_words.max() >= 3 and not np.isnan(score).any()
    assert not np.isin(words, [2, 5]).any() and not (words[:, 0] == 1).any()
    assert GR.forbidden_bigrams(words, n_words, enter, pair, leave) == 0
    for i in np.flatnonzero(n_words):
        k = n_words[i]
        assert start[i, 0] == 0 and (np.diff(start[i, :k]) > 0).all() and (words[i, k:] == -1).all()
    same(GR.decode(model, sym, n, None, pair, None, form="rows"), GR.decode(model, sym, n, np.zeros(7), pair, np.zeros(7), form="table"))


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_the_two_forms_agree_on_the_tie_corpus(seed):
    """A condition on the input as well: at least 8 % of the finite G(t, c) have their minimum in two or more
    predecessors."""
    model, enter, sym, n = R.tie_corpus(seed, N=12)
    pair, leave = GR.tie_grammar(seed)
    stats = [0, 0]
    rows = GR.decode(model, sym, n, enter, pair, leave, form="rows", stats=stats)
    print("finite G %d, shared %.3f" % (stats[0], stats[1] / stats[0]))
    assert stats[0] > 3000 and stats[1] / stats[0] >= 0.08, stats
    same(rows, GR.decode(model, sym, n, enter, pair, leave, form="table"))
    assert np.isfinite(rows[0]).all() and rows[1].min() >= 1 and rows[1].max() >= 3
    assert GR.forbidden_bigrams(rows[2], rows[1], enter, pair, leave) == 0


def brute_force(row, model, enter, pair, leave):
    """(cost, words, starts) over every word sequence and state path, each path costed left to right in the
    recurrence's own association: e + (prev + trans) inside a word, e + (0.0 + enter) at frame 0,
    e + (prev + pair) at a word change, then prev + leave.  Among the paths of the smallest cost the walk-back
    order decides: compared from the last frame backwards, the smaller last model, then at every frame staying
    before having advanced or entered, and at a boundary the smaller model before it."""
    n, C = len(row), len(model.n_states)
    ms = [model.one(c) for c in range(C)]
    best = [None]

    def step(t, c, s, prev, key, words):
        if t == n:
            total = prev + np.float64(leave[c])
            if s == len(ms[c][1]) - 1 and total < INF:
                if best[0] is None or (total, (c,) + key) < best[0][:2]:
                    best[0] = (total, (c,) + key, list(words))
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
            if t == 0:
                opts.append((0, enter[c2], (1, -1), True))
            elif s == len(ms[c][1]) - 1:
                opts.append((0, pair[c, c2], (1, c), True))
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
    rng = np.random.default_rng(61 if corpus == "dyadic" else 62)
    several = finite = 0
    for case in range(100):
        C, Smax, K = int(rng.integers(1, 4)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
        states = rng.integers(1, Smax + 1, C).astype(np.int32)
        if corpus == "dyadic":
            model = D.Model(rng.integers(0, 4, (C, Smax, K)) / 2.0, rng.integers(0, 3, (C, Smax)) / 2.0,
                            rng.integers(0, 3, (C, Smax)) / 2.0, states)
            enter, pair, leave = rng.integers(0, 4, C) / 2.0, rng.integers(0, 4, (C, C)) / 2.0, rng.integers(0, 3, C) / 2.0
        else:
            model = D.random_models(states, Smax, K, seed=100 + case)
            enter, pair, leave = rng.uniform(0, 2, C), rng.uniform(0, 2, (C, C)), rng.uniform(0, 2, C)
        pair[rng.random((C, C)) < 0.2] = INF
        if case % 7 == 0:
            enter[rng.integers(0, C)] = INF
        if case % 5 == 0:
            leave[rng.integers(0, C)] = INF
        n = int(rng.integers(1, 7))
        row = [int(k) for k in rng.integers(0, K, n)]
        want = brute_force(row, model, enter, pair, leave)
        for form in ("table", "rows"):
            score, found = GR.decode_one(row, model, enter, pair, leave, form)
            assert bits(score) == bits(want[0]), (case, form)
            assert [w for w, _ in found] == want[1] and [b for _, b in found] == want[2], (case, form, found, want)
        several += len(want[1]) > 1
        finite += np.isfinite(want[0])
    print(corpus, several, finite)
    assert several >= 15 and finite >= 50


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_a_free_loop_grammar_is_the_loop_decoder(seed):
    """(a) pair[p, c] = enter[c] for all p with leave NULL gives dhmm_decode_reference.decode's score, words and
    starts -- on the dyadic corpus only: with real costs two different exits can round to the same sum."""
    model, enter, sym, n = R.tie_corpus(seed)
    want = R.decode(model, sym, n, enter)
    got = GR.decode(model, sym, n, *GR.loop_grammar(enter, 10))
    same(got, want[:4])
    assert want[1].max() >= 3


def chain_cases(model, enter, sym, n, seed, Wmax=4):
    """Transcripts of 1 .. Wmax DISTINCT words of the ten models for the tie corpus' utterances."""
    rng = np.random.default_rng(seed)
    trans = np.full((len(n), Wmax), -1, np.int32)
    L = rng.integers(1, Wmax + 1, len(n)).astype(np.int32)
    for u in range(len(n)):
        trans[u, :L[u]] = rng.permutation(len(model.n_states))[:L[u]]
    return trans, L


def test_a_chain_grammar_is_the_forced_alignment():
    """(b) the chain grammar of a transcript of distinct words gives dhmm_force_reference's forced score, the
    words equal to the transcript and start[i] = seg[i][0]; where the forced score is +inf, +inf and 0 words."""
    model, enter, sym, n = R.tie_corpus(2, N=24)
    n[:4] = [3, 5, 8, 12]  # some too short for their chain
    trans, L = chain_cases(model, enter, sym, n, seed=70)
    score, seg = F.align(model, sym, n, trans, L, enter)
    assert np.isinf(score).sum() >= 1 and np.isfinite(score).sum() >= 18 and (L >= 3).sum() >= 6
    for u in range(len(n)):
        words = [int(w) for w in trans[u, :L[u]]]
        got = GR.decode(model, sym[u:u + 1], n[u:u + 1], *GR.chain_grammar(words, enter, 10), max_words=4)
        assert bits(got[0][0]) == bits(score[u]), u
        if score[u] < INF:
            assert got[1][0] == L[u] and list(got[2][0, :L[u]]) == words
            assert np.array_equal(got[3][0, :L[u]], seg[u, :L[u], 0])
        else:
            assert got[1][0] == 0 and (got[2] == -1).all()


def test_a_closed_grammar_decodes_one_word():
    """(c) pair all +inf: every finite result is one word, and its score is the smallest
    isolated score + enter + leave -- as (e + (0.0 + enter)) ... + leave, the isolated Viterbi's sums with the
    entry cost in front: checked on the dyadic corpus, where every sum is exact."""
    model, enter, sym, n = R.tie_corpus(3)
    n[:6] = [1, 2, 3, 5, 8, 8]
    leave = np.random.default_rng(5).integers(0, 3, 10) / 2
    score, n_words, words, start = GR.decode(model, sym, n, enter, np.full((10, 10), INF), leave)
    iso = D.score(model, sym, n)[0] + enter[None, :] + leave[None, :]
    assert np.array_equal(bits(score), bits(iso.min(axis=1)))
    assert np.array_equal(n_words, np.isfinite(score)) and np.isfinite(score).sum() >= 20
    assert np.array_equal(words[:, 0], D.label_of(iso)) and (start[n_words > 0, 0] == 0).all()


def test_no_output_breaks_the_grammar():
    """(d) on real-valued models and a sparse grammar, with a ban on repeating a word."""
    model = R.word_models(8, 4, 12, seed=80)
    sym, n = D.random_symbols(30, 40, 12, seed=81, lo=5)
    enter, pair, leave = GR.random_grammar(8, seed=82, forbid=0.5)
    pair[np.arange(8), np.arange(8)] = INF
    enter[[0, 3]] = leave[[1, 2]] = INF
    score, n_words, words, start = GR.decode(model, sym, n, enter, pair, leave)
    assert np.isfinite(score).sum() >= 15 and n_words.max() >= 4
    assert GR.forbidden_bigrams(words, n_words, enter, pair, leave) == 0
    free = R.decode(model, sym, n, np.zeros(8))
    assert GR.forbidden_bigrams(free[2], free[1], enter, pair, leave) > 0  # the free loop does break it


def test_word_pair_grammar_from_transcripts():
    """Three words, four utterances, by hand: first = [2, 1, 0] (a fifth, empty, utterance is skipped),
    bigrams 0>1 x2, 1>2 x2, 1>1 x1, ends on 2 x2, on 1 x1, on 0 x1."""
    from src.models import WordPairGrammar
    trans = [[0, 1, 2], [0, 1, 1, 2], [1], [], [0]]
    g = WordPairGrammar.from_transcripts(trans, 3, alpha=0.5)
    assert np.array_equal(bits(g.enter), bits(-np.log(np.array([3 + 0.5, 1 + 0.5, 0 + 0.5]) / (4 + 1.5))))
    n = np.array([[0, 2, 0], [0, 1, 2], [0, 0, 0]], np.float64)
    end = np.array([1, 1, 2], np.float64)
    row = n.sum(axis=1) + end + 0.5 * 4
    assert np.array_equal(row, [5, 6, 4])
    assert np.array_equal(bits(g.pair), bits(-np.log((n + 0.5) / row[:, None])))
    assert np.array_equal(bits(g.leave), bits(-np.log((end + 0.5) / row)))
    # a row and its end event are one distribution
    assert np.allclose(np.exp(-g.pair).sum(axis=1) + np.exp(-g.leave), 1.0) and np.isclose(np.exp(-g.enter).sum(), 1.0)
    g0 = WordPairGrammar.from_transcripts(trans, 3, alpha=0)
    assert np.array_equal(np.isinf(g0.pair), n == 0) and np.array_equal(np.isinf(g0.enter), [False, False, True])
    assert bits(g0.pair[1, 2]) == bits(-np.log(np.float64(2) / np.float64(4))) and not np.isnan(g0.pair).any()
    assert np.isinf(WordPairGrammar.from_transcripts([[0]], 3, alpha=0).pair).all()  # rows without an event
    with pytest.raises(ValueError):
        WordPairGrammar.from_transcripts([[0, 3]], 3)


def test_word_pair_grammar_from_allowed_and_plus():
    from src.models import WordPairGrammar
    follows = np.array([[0, 1, 1], [0, 0, 1], [1, 0, 0]], bool)
    g = WordPairGrammar.from_allowed(follows, first=[1, 0, 0], last=None)
    assert np.array_equal(g.pair, np.where(follows, 0.0, INF)) and np.array_equal(g.enter, [0.0, INF, INF])
    assert np.array_equal(g.leave, np.zeros(3)) and g.n_classes == 3
    h = g.plus([1.0, 2.0, 0.5])
    assert np.array_equal(h.enter, [1.0, INF, INF]) and np.array_equal(h.leave, g.leave)
    assert np.array_equal(h.pair, np.where(follows, np.array([1.0, 2.0, 0.5])[None, :], INF))
    assert np.array_equal(g.plus(0.25).pair, np.where(follows, 0.25, INF)) and np.array_equal(g.pair, np.where(follows, 0.0, INF))
    with pytest.raises(ValueError):
        WordPairGrammar(None, np.full((2, 2), np.nan), None)
    with pytest.raises(ValueError):
        WordPairGrammar(None, np.zeros((2, 3)), None)


def test_decode_surface_without_a_device():
    import inspect

    from src.models import DiscreteHmmClassifier
    from src.pipeline import dhmm_decode_grammar
    assert callable(dhmm_decode_grammar)
    assert inspect.signature(DiscreteHmmClassifier.decode).parameters["grammar"].default is None


def test_abi_argument_checks():
    """The plan's bounds and the NULL checks, answered on the host before any launch."""
    from src import _hip
    lib = _hip.load_library()
    for name in ("dsp_dhmm_decode_grammar_workspace_bytes", "dsp_dhmm_decode_grammar"):
        assert name in _hip.EXPORTS and hasattr(lib, name)
    wb = lib.dsp_dhmm_decode_grammar_workspace_bytes
    base = lib.dsp_dhmm_decode_workspace_bytes
    # the decoder's transposed set, then a 32-bit word per frame and lane for each persistent wave (groups of four)
    assert wb(10, 5, 64, 8, 64) == base(10, 5, 64, 8, 64) + 8 * 64 * 256
    assert wb(64, 100, 1024, 32, 256) == base(64, 100, 1024, 32, 256) + 100 * 1024 * 256
    assert wb(64, 5000, 1024, 32, 256) == base(64, 5000, 1024, 32, 256) + (256 << 20)  # the waves are capped
    assert wb(3, 100000, 6, 5, 16) == base(3, 100000, 6, 5, 16) + 8192 * 6 * 256 and wb(1, 0, 1, 1, 1) > 0
    for args in ((65, 4, 64, 5, 64), (0, 4, 64, 5, 64), (-1, 4, 64, 5, 64), (3, 4, 1025, 5, 64), (3, 4, 0, 5, 64),
                 (3, 4, 64, 5, 257), (3, 4, 64, 5, 0), (3, 4, 64, 33, 64), (3, 4, 64, 0, 64), (3, -1, 64, 5, 64)):
        assert wb(*args) == 0, args
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30

    def call(C=3, Smax=5, K=64, N=4, T=64, max_words=4, emit=p, pair=p, sym=p, outs=(p, p, p, p), ws=p, nws=big):
        return lib.dsp_dhmm_decode_grammar(emit, p, p, p, None, pair, None, C, Smax, K, sym, p, N, T, max_words, *outs, ws, nws,
                                           None)

    for bad in (dict(pair=None), dict(C=65), dict(C=0), dict(T=1025), dict(T=0), dict(K=257), dict(K=0), dict(Smax=33),
                dict(Smax=0), dict(max_words=0), dict(max_words=65), dict(N=-1), dict(emit=None), dict(sym=None)):
        assert call(**bad) == _hip.DSP_ERR_ARGS, bad
    assert call(ws=None, nws=0) == _hip.DSP_ERR_WORKSPACE and call(nws=wb(3, 4, 64, 5, 64) - 1) == _hip.DSP_ERR_WORKSPACE
    assert call(N=0, ws=None, nws=0) == _hip.DSP_OK
    assert call(outs=(None,) * 4, ws=None, nws=0) == _hip.DSP_OK
    assert call(N=0, C=65) == _hip.DSP_ERR_ARGS  # the bounds come before "nothing to do"
