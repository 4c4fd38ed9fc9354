"""CPU tests of the forced-alignment definition (tests/dhmm_force_reference.py) and of the host side on it:
the two forms of the restatement agree bit for bit, the result is the brute force's over all monotone state
paths of the chain, the consequences of the definition against the isolated-word Viterbi of
tests/dhmm_reference.py and the decoder of tests/dhmm_decode_reference.py, the embedded re-estimate's counts,
the flat start, one round of embedded training, and the argument checks that need no device."""
import ctypes

import numpy as np
import pytest

import dhmm_decode_reference as R
import dhmm_force_reference as F
import dhmm_reference as D

INF = np.inf


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def same(got, want):
    assert np.array_equal(bits(got[0]), bits(want[0])), ("score", np.argwhere(bits(got[0]) != bits(want[0]))[:5])
    assert np.array_equal(got[1], want[1]), ("seg", np.argwhere(got[1] != want[1])[:5])


def random_corpus():
    """dhmm_decode's host corpus -- seven models (one with n_states 0, one with Smax + 1) over K = 9 symbols
    with a +inf emission, an all-+inf emission row, a +inf stay and +inf entry costs; 40 utterances of up to 30
    frames, three with a symbol outside the alphabet, two with a bad length -- with transcripts of 1 .. 4
    words: the models 2 (n_states 0) and 5 (Smax + 1) inside some, word counts 0 and Wmax + 1, indices -1 and
    C."""
    model = D.random_models(np.array([3, 1, 0, 5, 2, 6, 4], np.int32), 5, 9, seed=5)
    model.emit[0, 1, 3] = model.emit[3, 2, :] = model.stay[4, 0] = INF
    model.emit[[2, 5]] = np.nan  # never read
    enter = np.array([0.5, 2.0, 0.0, INF, 0.0, 1.0, 0.25])
    sym, n = D.random_symbols(40, 30, 9, seed=6)
    sym[3, 0], sym[4, n[4] - 1], sym[5, n[5] // 2] = 9, -1, 2 ** 31 - 1
    n[[7, 8]] = [0, 31]
    trans, L = F.random_transcripts(40, 4, 7, seed=7)
    trans[np.isin(trans, [2, 5])] = 1
    trans[20:][trans[20:] == 3] = 6  # the word that is never entered stays in the first half only
    trans[10, 0], trans[11, L[11] - 1], trans[12, 0], trans[13, L[13] - 1] = 2, 5, -1, 7
    L[[14, 15]] = [0, 5]
    return model, enter, sym, n, trans, L


FORCED = [3, 4, 5, 7, 8, 10, 11, 12, 13, 14, 15]


def test_the_two_forms_agree():
    model, enter, sym, n, trans, L = random_corpus()
    table = F.align(model, sym, n, trans, L, enter, form="table")
    same(F.align(model, sym, n, trans, L, enter, form="rows"), table)
    score, seg = table
    assert np.isinf(score[FORCED]).all() and (seg[FORCED] == -1).all() and not np.isnan(score).any()
    assert np.isfinite(score).sum() >= 12 and (np.isfinite(score) & (L >= 3)).sum() >= 4
    for u in np.flatnonzero(np.isfinite(score)):
        S = model.n_states[trans[u, :L[u]]]
        chain = np.concatenate([seg[u, i, :S[i]] for i in range(L[u])])
        assert chain[0] == 0 and (np.diff(chain) > 0).all() and chain[-1] < n[u]
        assert (seg[u, L[u]:] == -1).all() and all((seg[u, i, S[i]:] == -1).all() for i in range(L[u]))
        assert 3 not in trans[u, 1:L[u]]  # enter +inf: never entered behind another word
    assert (seg[np.isinf(score)] == -1).all()
    same(F.align(model, sym, n, trans, L, None, form="rows"), F.align(model, sym, n, trans, L, np.zeros(7), form="table"))


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_the_two_forms_agree_on_the_tie_corpus(seed):
    """A condition on the input as well: the share of decided cells with a == b.  Measured on the seeds 1, 2,
    3: 0.090, 0.098, 0.092; the floor asserted is 0.04, under half the smallest."""
    model, enter, sym, n, trans, L = F.tie_corpus(seed)
    stats = [0, 0]
    rows = F.align(model, sym, n, trans, L, enter, form="rows", stats=stats)
    print("cells %d tied %.3f" % (stats[0], stats[1] / stats[0]))
    assert stats[0] > 5000 and stats[1] / stats[0] >= 0.04, stats
    same(rows, F.align(model, sym, n, trans, L, enter, form="table"))
    assert np.isfinite(rows[0]).sum() >= 20


@pytest.mark.parametrize("corpus", ("dyadic", "random"))
def test_the_result_is_the_brute_force_minimum(corpus):
    """120 tiny cases each (n <= 8, L <= 3, S <= 3): the score is the smallest path cost bit for bit and seg is
    one of the paths that reach it; where every sum is exact it is the one the tie rule names."""
    rng = np.random.default_rng(61 if corpus == "dyadic" else 62)
    finite = several = 0
    for case in range(120):
        C, Smax, K = int(rng.integers(1, 4)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
        states = rng.integers(1, Smax + 1, C).astype(np.int32)
        if corpus == "dyadic":
            model = D.Model(rng.integers(0, 4, (C, Smax, K)) / 2.0, rng.integers(0, 3, (C, Smax)) / 2.0,
                            rng.integers(0, 3, (C, Smax)) / 2.0, states)
            enter = rng.integers(0, 4, C) / 2.0
        else:
            model, enter = D.random_models(states, Smax, K, seed=300 + case), rng.uniform(0, 2, C)
        if case % 9 == 0:
            enter[rng.integers(0, C)] = INF
        words = [int(w) for w in rng.integers(0, C, int(rng.integers(1, 4)))]
        row = [int(k) for k in rng.integers(0, K, int(rng.integers(1, 9)))]
        cost = R.enter_of(model, enter)
        best, paths = F.brute_force(row, model, cost, words)
        for form in ("table", "rows"):
            score, seg = F.force_table(row, model, cost, words) if form == "table" else F.force_rows(row, model, cost, words, 3)
            assert bits(score) == bits(best), (case, form)
            if best < INF:
                chosen = tuple(f for firsts in seg for f in firsts)
                assert chosen in paths, (case, form, seg, paths)
                if corpus == "dyadic":  # exact sums: ties stay, so from the last state backwards each begins as early as it can
                    assert chosen[::-1] == min(p[::-1] for p in paths), (case, form, seg, paths)
            else:
                assert seg is None
        finite += best < INF
        several += len(paths) > 1
    print(corpus, finite, several)
    assert finite >= 50 and (corpus == "random" or several >= 15)


def test_a_single_word_is_the_isolated_alignment():
    """(a) L = 1 and enter = 0: score and seg are dsp_dhmm_align's isolated Viterbi score and seg row."""
    model = D.random_models(np.array([4, 5, 1, 6], np.int32), 6, 11, seed=41)
    sym, n = D.random_symbols(40, 12, 11, seed=42, lo=1)
    word = np.arange(40, dtype=np.int32) % 4
    score, seg = F.align(model, sym, n, word[:, None], np.ones(40, np.int32), np.zeros(4))
    order = np.argsort(word, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(word, minlength=4))])
    iso, iso_seg = D.align(model, sym, n, start, order)
    assert np.array_equal(bits(score[order]), bits(iso)) and np.array_equal(seg[order, 0], iso_seg)
    assert np.isfinite(score).sum() >= 25 and np.isinf(score).sum() >= 3


def decoded_corpus():
    model = D.random_models(np.array([2, 3, 1, 4], np.int32), 4, 6, seed=43)
    enter = np.array([0.5, 0.25, 1.5, 0.0])
    sym, n = D.random_symbols(30, 25, 6, seed=44, lo=8)
    return model, enter, sym, n, R.decode(model, sym, n, enter)


def test_forcing_the_decoded_words_gives_the_decoded_score():
    """(b) the fp additions are monotone, so the minimum over the transcript's paths is the minimum the decoder
    found over all word sequences; any other transcript of the same utterance scores no less.  (c) on this
    non-dyadic corpus the forced word starts are the decoder's: both restatements confirm it here, so it is
    asserted."""
    model, enter, sym, n, (score, n_words, words, start, _) = decoded_corpus()
    Wmax = int(n_words.max())
    assert Wmax >= 4 and n_words.min() >= 1
    for form in ("rows", "table"):
        got, seg = F.align(model, sym, n, words[:, :Wmax], n_words, enter, form=form)
        assert np.array_equal(bits(got), bits(score)), form
        assert np.array_equal(seg[:, :, 0], start[:, :Wmax]), form
    other, L = F.random_transcripts(30, Wmax, 4, seed=45)
    got, _ = F.align(model, sym, n, other, L, enter)
    assert (got >= score).all() and (got > score).sum() >= 20


def counting_corpus():
    model = R.word_models(5, 4, 7, seed=70, states=[2, 4, 1, 3, 4])
    sym, n = D.random_symbols(30, 40, 7, seed=71, lo=10)
    trans, L = F.random_transcripts(30, 4, 5, seed=72)
    _, seg = F.align(model, sym, n, trans, L, np.full(5, 0.5))
    return model, sym, n, trans, L, seg


def test_accumulate_counts():
    model, sym, n, trans, L, seg = counting_corpus()
    sym[5, 3], n[6], L[7], trans[8, 0] = 7, 41, 0, 5  # a symbol outside the alphabet, a bad length, no word, a bad word
    cnt_emit, cnt, n_valid, valid = F.accumulate(model.n_states, 7, sym, n, trans, L, seg)
    assert not valid[[5, 6, 7, 8]].any() and valid.sum() >= 20
    assert np.array_equal(valid != 0, (seg[:, 0, 0] == 0) & ~np.isin(np.arange(30), [5, 6, 7, 8]))
    assert np.array_equal(cnt_emit.sum(axis=2), cnt) and cnt.sum() == n[valid != 0].sum()
    hist = np.zeros(5, np.int64)
    for u in np.flatnonzero(valid):
        hist += np.bincount(trans[u, :L[u]], minlength=5)
    assert np.array_equal(n_valid, hist) and (n_valid > 0).all()
    assert all((cnt[c, model.n_states[c]:] == 0).all() for c in range(5))
    # the counts again, frame by frame from the seg rows' own run ends
    again = np.zeros_like(cnt_emit)
    for u in np.flatnonzero(valid):
        chain = [(trans[u, i], s, seg[u, i, s]) for i in range(L[u]) for s in range(model.n_states[trans[u, i]])]
        for j, (w, s, b) in enumerate(chain):
            for t in range(b, chain[j + 1][2] if j + 1 < len(chain) else n[u]):
                again[w, s, sym[u, t]] += 1
    assert np.array_equal(again, cnt_emit)


def test_accumulate_skips_malformed_rows_whole():
    model, sym, n, trans, L, seg = counting_corpus()
    good = np.flatnonzero((seg[:, 0, 0] == 0) & (L >= 2) & (seg == -1).any(axis=(1, 2)))[:5]
    assert len(good) == 5
    base = F.accumulate(model.n_states, 7, sym, n, trans, L, seg)
    seg = seg.copy()
    u0, u1, u2, u3, u4 = good
    last = lambda u, i: model.n_states[trans[u, i]] - 1
    seg[u0, 0, 0] = 1                              # not starting at 0
    seg[u1, 1, 0] = seg[u1, 0, last(u1, 0)]        # a repeated frame
    seg[u2, L[u2] - 1, last(u2, L[u2] - 1)] = n[u2]  # a last frame >= n
    i, s = np.argwhere(seg[u3] == -1)[0]
    seg[u3, i, s] = n[u3] - 1                      # an entry where the definition says -1
    seg[u4, 1, 0] = -1                             # a stray -1 inside the chain
    cnt_emit, cnt, n_valid, valid = F.accumulate(model.n_states, 7, sym, n, trans, L, seg)
    assert not valid[good].any() and valid.sum() == base[3].sum() - 5
    keep = np.ones(30, bool)
    keep[good] = False
    want = F.accumulate(model.n_states, 7, sym[keep], n[keep], trans[keep], L[keep], seg[keep])
    assert all(np.array_equal(g, w) for g, w in zip((cnt_emit, cnt, n_valid), want[:3]))


def test_the_flat_start_by_hand():
    from src.pipeline import dhmm_flat_segmentation
    states = np.array([2, 3, 1], np.int32)
    trans = np.array([[0, 1, -7], [2, 2, 2], [1, 0, 3], [0, 1, 2], [1, 2, 0]], np.int32)
    L = np.array([2, 3, 3, 3, 4], np.int32)
    n = np.array([12, 7, 20, 5, 20], np.int32)
    want = np.full((5, 3, 3), -1, np.int32)
    want[0, 0, :2], want[0, 1, :3] = [0, 2], [4, 7, 9]  # J = 5, n = 12: floor(12 j / 5)
    want[1, :, 0] = [0, 2, 4]                           # J = 3, n = 7: floor(7 j / 3)
    got = dhmm_flat_segmentation(n, trans, L, states, 3)  # row 2: word 3 is no model; row 3: n = 5 < J = 6; row 4: L > Wmax
    assert np.array_equal(got, want) and np.array_equal(F.flat_segmentation(n, trans, L, states, 3), want)
    rng = np.random.default_rng(80)
    states = rng.integers(0, 7, 9).astype(np.int32)  # a 0 and a 6 > Smax = 5 among them
    trans, L = F.random_transcripts(200, 6, 9, seed=81, lo=0)
    L[:3] = [7, -1, 0]
    n = rng.integers(0, 60, 200).astype(np.int32)
    got = dhmm_flat_segmentation(n, trans, L, states, 5)
    assert np.array_equal(got, F.flat_segmentation(n, trans, L, states, 5)) and (got[:, 0, 0] == 0).sum() >= 20
    lists = dhmm_flat_segmentation(n[3:], [trans[u, :L[u]] for u in range(3, 200)], None, states, 5)
    assert lists.shape[1] == L[3:].max() and np.array_equal(lists, got[3:, :lists.shape[1]])


def spoken_corpus(seed, N=24):
    """Utterances of 2 .. 4 words over K = 8 symbols: word c is three stretches of 2 .. 5 frames, each drawn
    mostly from its own symbol -- concatenations of isolated sequences, their boundaries forgotten."""
    rng = np.random.default_rng(seed)
    main = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 0], [2, 5, 7]])
    rows, trans = [], []
    for _ in range(N):
        words = rng.integers(0, 4, int(rng.integers(2, 5)))
        row = [int(main[w, p]) if rng.random() < 0.8 else int(rng.integers(0, 8))
               for w in words for p in range(3) for _ in range(int(rng.integers(2, 6)))]
        rows.append(row)
        trans.append(words)
    n = np.array([len(r) for r in rows], np.int32)
    sym = np.full((N, int(n.max())), -1, np.int32)
    for i, r in enumerate(rows):
        sym[i, :len(r)] = r
    L = np.array([len(w) for w in trans], np.int32)
    tr = np.full((N, 4), -1, np.int32)
    for i, w in enumerate(trans):
        tr[i, :len(w)] = w
    return sym, n, tr, L


def test_a_round_of_embedded_training_does_not_raise_the_total():
    sym, n, trans, L = spoken_corpus(90)
    states = np.full(4, 3, np.int32)
    model, totals, seg = F.fit_connected(sym, n, trans, L, states, 8, n_iter=3)
    assert len(totals) >= 2 and totals[1] <= totals[0] and np.isfinite(totals).all()
    again = F.fit_connected(sym, n, trans, L, states, 8, n_iter=3, form="table")
    assert np.array_equal(bits(again[1]), bits(totals)) and np.array_equal(again[2], seg)
    assert all(np.array_equal(bits(getattr(again[0], f)), bits(getattr(model, f))) for f in ("emit", "stay", "adv"))
    # the word starts the training found are mostly the true ones: three stretches a word, 2 .. 5 frames each
    assert (seg[:, 0, 0] == 0).all()
    # word 3 only in an utterance shorter than its chain of 4 x 3 states: no instance is left for it
    trans, L, n = np.where(trans == 3, 0, trans), L.copy(), n.copy()
    trans[0], L[0], n[0] = 3, 4, 11
    with pytest.raises(ValueError):
        F.fit_connected(sym, n, trans, L, states, 8)


def test_python_argument_checks_without_a_device():
    from src.models import DiscreteHmmClassifier
    from src.pipeline import (DHMM_FORCE_MAX_WORDS, DhmmModelSet, VqTokenizer, dhmm_flat_segmentation, dhmm_force_align)
    assert DHMM_FORCE_MAX_WORDS == F.MAX_WORDS == 64
    m = D.random_models(np.full(65, 2, np.int32), 2, 4, seed=1)
    big = DhmmModelSet.from_arrays(m.emit, m.stay, m.adv, m.n_states)
    sym, n = np.zeros((2, 5), np.int32), np.array([5, 5])
    with pytest.raises(ValueError, match="word models"):
        dhmm_force_align(big, sym, n, [[0], [1]])
    ok = DhmmModelSet.from_arrays(m.emit[:3], m.stay[:3], m.adv[:3], m.n_states[:3])
    with pytest.raises(ValueError, match="words"):
        dhmm_force_align(ok, sym, n, [[0] * 65, [1]])
    with pytest.raises(ValueError, match="transcripts"):
        dhmm_force_align(ok, sym, n, [[0]])
    with pytest.raises(ValueError, match="Wmax"):
        dhmm_force_align(ok, sym, n, np.zeros((2, 3, 1), np.int32), n_trans=[1, 1])
    with pytest.raises(ValueError):
        dhmm_flat_segmentation(n, np.zeros((2, 65), np.int32), [1, 1], [2, 2, 2], 2)
    X = [np.zeros((6, 2)), np.ones((7, 2))]
    with pytest.raises(ValueError, match="Baum-Welch"):
        DiscreteHmmClassifier(training='baum_welch').fit_connected(X, [["a"], ["b"]])
    with pytest.raises(ValueError, match="transcripts for"):
        DiscreteHmmClassifier().fit_connected(X, [["a"]])
    with pytest.raises(ValueError, match="empty transcript"):
        DiscreteHmmClassifier().fit_connected(X, [["a"], []])
    with pytest.raises(ValueError, match="at most 64"):
        DiscreteHmmClassifier(n_states=1).fit_connected(X, [list(range(40)), list(range(30, 70))])
    with pytest.raises(ValueError, match="n_states for"):
        DiscreteHmmClassifier(n_states=[2, 2, 2]).fit_connected(X, [["a"], ["b"]])
    clf = DiscreteHmmClassifier(n_codes=4, normalize=False)
    clf.classes_, clf.tokenizer_ = np.array(["a", "b"]), VqTokenizer(4)
    clf.tokenizer_.codebook_ = np.zeros((4, 2))
    with pytest.raises(ValueError, match="not one of the fitted classes"):
        clf.align(X, [["a", "b"], ["a", "c"]])
    with pytest.raises(ValueError, match="transcripts for"):
        clf.align(X, [["a"]])
    with pytest.raises(ValueError, match="feature channels"):
        clf.align([np.zeros((6, 3))], [["a"]])


def test_abi_argument_checks():
    """The plan's bounds and the NULL checks, answered on the host before any launch."""
    from src import _hip
    lib = _hip.load_library()
    wb = lib.dsp_dhmm_force_workspace_bytes  # (C, N, T, Wmax, Smax, K)
    assert wb(64, 100, 1024, 64, 32, 256) >= 256 * 32 * 64 * 8 + 100 * 1024 * 256 and wb(1, 0, 1, 1, 1, 1) > 0
    assert wb(10, 5, 64, 4, 8, 64) < wb(10, 5, 64, 4, 9, 64) < wb(10, 5, 64, 4, 17, 64)
    assert wb(10, 5, 64, 4, 8, 64) < wb(10, 6, 64, 4, 8, 64) and wb(10, 100000, 1024, 4, 8, 64) - wb(10, 1, 1024, 4, 8, 64) < 1 << 28
    for args in ((65, 4, 64, 4, 5, 64), (0, 4, 64, 4, 5, 64), (3, 4, 1025, 4, 5, 64), (3, 4, 0, 4, 5, 64), (3, 4, 64, 65, 5, 64),
                 (3, 4, 64, 0, 5, 64), (3, 4, 64, 4, 5, 257), (3, 4, 64, 4, 5, 0), (3, 4, 64, 4, 33, 64), (3, 4, 64, 4, 0, 64),
                 (3, -1, 64, 4, 5, 64)):
        assert wb(*args) == 0, args
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30

    def align(C=3, Smax=5, K=64, N=4, T=64, Wmax=4, emit=p, sym=p, trans=p, outs=(p, p), ws=p, nws=big):
        return lib.dsp_dhmm_force_align(emit, p, p, p, None, C, Smax, K, sym, p, N, T, trans, p, Wmax, *outs, ws, nws, None)

    def accumulate(C=3, Smax=5, K=64, N=4, T=64, Wmax=4, n_states=p, seg=p, outs=(p, p, p, p), ws=p, nws=big):
        return lib.dsp_dhmm_force_accumulate(n_states, C, Smax, K, p, p, N, T, p, p, Wmax, seg, *outs, ws, nws, None)

    for bad in (dict(C=65), dict(C=0), dict(T=1025), dict(T=0), dict(K=257), dict(K=0), dict(Smax=33), dict(Smax=0),
                dict(Wmax=0), dict(Wmax=65), dict(N=-1)):
        assert align(**bad) == _hip.DSP_ERR_ARGS and accumulate(**bad) == _hip.DSP_ERR_ARGS, bad
    for bad in (dict(emit=None), dict(sym=None), dict(trans=None)):
        assert align(**bad) == _hip.DSP_ERR_ARGS, bad
    for bad in (dict(n_states=None), dict(seg=None), dict(outs=(None, p, p, p)), dict(outs=(p, p, p, None))):
        assert accumulate(**bad) == _hip.DSP_ERR_ARGS, bad
    need = wb(3, 4, 64, 4, 5, 64)
    assert align(ws=None, nws=0) == _hip.DSP_ERR_WORKSPACE and align(nws=need - 1) == _hip.DSP_ERR_WORKSPACE
    assert accumulate(ws=None, nws=0) == _hip.DSP_ERR_WORKSPACE and accumulate(nws=need - 1) == _hip.DSP_ERR_WORKSPACE
    assert align(N=0, ws=None, nws=0) == _hip.DSP_OK and align(outs=(None, None), ws=None, nws=0) == _hip.DSP_OK
    assert align(N=0, C=65) == _hip.DSP_ERR_ARGS  # the bounds come before "nothing to do"
