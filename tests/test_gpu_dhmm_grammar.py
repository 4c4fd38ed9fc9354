"""GPU tests of csrc/dhmm_grammar.hip (dsp_dhmm_decode_grammar) through the bare C ABI, and of the Python
surface on it.  Everything is compared with the numpy restatement of tests/dhmm_grammar_reference.py on the raw
bits and the raw integers: there is no tolerance and no utterance is left out.  Every output sits between guard
rows, enter, pair and leave are followed by NaN, the lengths by garbage, and behind each utterance's length the
symbol rows hold garbage: -1, K, 2^31 - 1 and INT_MIN."""
import numpy as np
import pytest

import dhmm_decode_reference as R
import dhmm_grammar_reference as GR
import dhmm_reference as D
from device_outputs import Guarded, _dev, bits
from test_gpu_dhmm_decode import _after, decode_raw
from test_gpu_dhmm_force import force_raw

pytestmark = pytest.mark.gpu

INF = np.inf
NAMES = ("score", "n_words", "words", "start")


def grammar_raw(model, sym, n, enter, pair, leave, max_words=None, without=()):
    """dsp_dhmm_decode_grammar through the bare C ABI -> (score, n_words, words, start); the outputs named in
    ``without`` are passed as NULL and come back as None."""
    import torch
    from src import _hip
    N, T = sym.shape
    C, Smax, K = model.emit.shape
    mw = T if max_words is None else max_words
    keep = [_after(a, torch.float64, np.nan) for a in (model.emit, model.stay, model.adv)]
    keep += [_after(model.n_states, torch.int32, 1 << 20)]
    keep += [None if a is None else _after(a, torch.float64, np.nan) for a in (enter, pair, leave)]
    ts, tn = _after(sym, torch.int32, -5), _after(n, torch.int32, 1 << 20)
    outs = [Guarded((N,), torch.float64, -7.0), Guarded((N,), torch.int32, -9), Guarded((N, mw), torch.int32, -9),
            Guarded((N, mw), torch.int32, -9)]
    nbytes = _hip.lib().dsp_dhmm_decode_grammar_workspace_bytes(C, N, T, Smax, K)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = _hip.lib().dsp_dhmm_decode_grammar(*[_hip.ptr(t) for t in keep], C, Smax, K, _hip.ptr(ts), _hip.ptr(tn), N, T, mw,
                                            *[None if name in without else _hip.ptr(o.view) for name, o in zip(NAMES, outs)],
                                            _hip.ptr(ws), nbytes, _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    got = []
    for name, o in zip(NAMES, outs):
        v = o.get()
        if name in without:
            assert (v == o.fill).all(), name
            v = None
        got.append(v)
    return tuple(got)


def same(got, want):
    for g, w, name in zip(got, want, NAMES):
        if g is None:
            continue
        g, w = (bits(v) if v.dtype == np.float64 else v for v in (g, w))
        assert g.shape == w.shape and np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


def check(model, sym, n, enter, pair, leave, max_words=None):
    want = GR.decode(model, sym, n, enter, pair, leave, max_words)
    same(grammar_raw(model, sym, n, enter, pair, leave, max_words), want)
    assert GR.forbidden_bigrams(want[2], want[1], enter, pair, leave) == 0
    return want


@pytest.mark.parametrize("C", (1, 2, 3, 10, 63, 64))
def test_model_counts(C):
    model = R.word_models(C, 5, 64, seed=1200 + C)
    enter, pair, leave = GR.random_grammar(C, seed=1300 + C, forbid=0.3 if C > 1 else 0.0)
    sym, n = D.random_symbols(20, 40, 64, seed=1400 + C, lo=1)
    score, n_words = check(model, sym, n, enter, pair, leave)[:2]
    assert np.isfinite(score).sum() >= 15 and n_words.max() >= 2


EDGE = lambda S: [0, 1, 2, max(S - 1, 1), S, 2 * S, 63, 64, 65, 66, 67]


@pytest.mark.parametrize("Smax", (1, 5, 8, 16, 17, 32))
def test_state_shapes(Smax):
    """The 8-, 16- and 32-slot kernels with Smax at and just past a slot count; mixed n_states with a 0 and an
    Smax + 1 among them, whose tables and whose rows and columns of pair (and entries of enter and leave) are
    NaN; lengths 0, 1, 2, S - 1, S, 2 S, 63 .. 66 and T + 1."""
    rng = np.random.default_rng(1500 + Smax)
    states = rng.integers(1, Smax + 1, 10)
    states[[0, 3, 4, 7, 8, 9]] = [Smax, 0, Smax + 1, max(Smax // 2, 1), max(Smax // 8, 1), min(3, Smax)]
    model = R.word_models(10, Smax, 64, seed=1510 + Smax, states=states)
    enter, pair, leave = GR.random_grammar(10, seed=1520 + Smax, forbid=0.2)
    model.emit[[3, 4]] = model.stay[[3, 4]] = model.adv[[3, 4]] = np.nan  # never read
    for a in (enter, leave, pair, pair.T):
        a[[3, 4]] = np.nan
    lengths = np.concatenate([EDGE(Smax), rng.integers(1, 67, 12)])
    sym, n = D.random_symbols(len(lengths), 66, 64, seed=1530 + Smax, lengths=lengths)
    score, n_words, words = check(model, sym, n, enter, pair, leave)[:3]
    assert np.isinf(score[[0, 10]]).all() and np.isfinite(score).sum() >= 15 and not np.isin(words, [3, 4]).any()
    assert not np.isnan(score).any() and n_words.max() >= (2 if Smax > 1 else 30)


@pytest.mark.parametrize("K", (1, 2, 64, 256))
def test_alphabets(K):
    model = R.word_models(5, 6, K, seed=1600 + K)
    enter, pair, leave = GR.random_grammar(5, seed=1605 + K, forbid=0.2)
    sym, n = D.random_symbols(20, 30, K, seed=1610 + K, lo=1)
    sym[3, 0], sym[4, n[4] - 1], sym[5, n[5] // 2], sym[6, 0] = K, -1, 2 ** 31 - 1, -2 ** 31
    score = check(model, sym, n, enter, pair, leave)[0]
    assert np.isinf(score[[3, 4, 5, 6]]).all() and np.isfinite(score).sum() >= 12


def test_longest_utterance():
    """One utterance at T = 1024 with C = 64 and Smax = 32 (32 slots: the transitions and 32 KiB of pair in LDS,
    256 KiB of trace words a wave), and one frame short of it."""
    model = R.word_models(64, 32, 64, seed=1700)
    enter, pair, leave = GR.random_grammar(64, seed=1702, forbid=0.3)
    sym, n = D.random_symbols(2, 1024, 64, seed=1701, lengths=[1024, 1023])
    score, n_words = check(model, sym, n, enter, pair, leave)[:2]
    assert np.isfinite(score).all() and n_words.min() >= 5


@pytest.mark.parametrize("N", (1, 2, 65, 300, 8300))
def test_utterance_counts(N):
    """N = 8300 is more than the persistent grid of 8192 waves holds at T = 6: a wave takes a second utterance
    and writes its trace words over the first one's.  The 8300 are 83 distinct utterances, each a hundred
    times."""
    model = R.word_models(10, 5, 16, seed=1800)
    enter, pair, leave = GR.random_grammar(10, seed=1802, forbid=0.3)
    base = N if N < 1000 else 83
    sym, n = D.random_symbols(base, 12 if N < 1000 else 6, 16, seed=1801 + N, lo=0)
    want = GR.decode(model, sym, n, enter, pair, leave, 6)
    reps = N // base
    got = grammar_raw(model, np.tile(sym, (reps, 1)), np.tile(n, reps), enter, pair, leave, 6)
    same(got, [np.tile(w, (reps,) + (1,) * (w.ndim - 1)) for w in want])
    assert np.isfinite(want[0]).sum() >= base // 3


def test_more_utterances_than_waves_at_the_longest_utterance():
    """T = 1024: a wave's trace words are 256 KiB, so the workspace cap leaves 1 024 persistent waves; N = 1 100
    gives 76 of them a second utterance.  Two distinct utterances (1 024 and 1 001 frames), each 550 times."""
    model = R.word_models(10, 5, 16, seed=1850)
    enter, pair, leave = GR.random_grammar(10, seed=1852, forbid=0.3)
    sym, n = D.random_symbols(2, 1024, 16, seed=1851, lengths=[1024, 1001])
    want = GR.decode(model, sym, n, enter, pair, leave, 8)
    assert np.isfinite(want[0]).all() and want[1].min() > 8
    got = grammar_raw(model, np.tile(sym, (550, 1)), np.tile(n, 550), enter, pair, leave, 8)
    same(got, [np.tile(w, (550,) + (1,) * (w.ndim - 1)) for w in want])


@pytest.mark.parametrize("seed", (1, 2))
def test_tie_rule(seed):
    """The dyadic tie corpus: the strict < of the cells, of the (min, +) step and of the end decide."""
    model, enter, sym, n = R.tie_corpus(seed, N=12)
    pair, leave = GR.tie_grammar(seed)
    stats = [0, 0]
    want = GR.decode(model, sym, n, enter, pair, leave, stats=stats)
    assert stats[1] / stats[0] >= 0.08, stats
    same(grammar_raw(model, sym, n, enter, pair, leave), want)
    assert np.isfinite(want[0]).all()


def test_a_free_loop_grammar_is_the_loop_decoder_on_the_device():
    """(a) pair[p, c] = enter[c] for all p, leave NULL: dsp_dhmm_decode's score, words and starts, both calls on
    the device, on the dyadic corpus."""
    model, enter, sym, n = R.tie_corpus(3)
    want = decode_raw(model, sym, n, enter)
    got = grammar_raw(model, sym, n, *GR.loop_grammar(enter, 10))
    same(got, want[:4])
    assert want[1].max() >= 3 and np.isfinite(want[0]).all()


def test_a_chain_grammar_is_the_forced_alignment_on_the_device():
    """(b) the chain grammar of a transcript of distinct words against dsp_dhmm_force_align on the device: the
    forced score, the transcript's words, start[i] = seg[i][0]; +inf and no word where the forced score is +inf."""
    model, enter, sym, n = R.tie_corpus(2, N=12)
    n[:3] = [3, 5, 8]  # too short for some chains
    rng = np.random.default_rng(1900)
    trans, L = np.full((12, 4), -1, np.int32), rng.integers(1, 5, 12).astype(np.int32)
    for u in range(12):
        trans[u, :L[u]] = rng.permutation(10)[:L[u]]
    score, seg = force_raw(model, sym, n, trans, L, enter)
    assert np.isinf(score).any() and np.isfinite(score).sum() >= 8
    for u in range(12):
        words = [int(w) for w in trans[u, :L[u]]]
        got = grammar_raw(model, sym[u:u + 1], n[u:u + 1], *GR.chain_grammar(words, enter, 10), max_words=4)
        assert bits(got[0][0]) == bits(score[u]), u
        if score[u] < INF:
            assert got[1][0] == L[u] and list(got[2][0, :L[u]]) == words and np.array_equal(got[3][0, :L[u]], seg[u, :L[u], 0])
        else:
            assert got[1][0] == 0 and (got[2] == -1).all() and (got[3] == -1).all()


def test_closed_grammars():
    """pair all +inf: one word, the smallest isolated score + enter + leave (exact on the dyadic corpus); enter
    all +inf and leave all +inf: nothing; a self-loop ban: no word twice in a row."""
    model, enter, sym, n = R.tie_corpus(3, N=12)
    n[:4] = [1, 2, 3, 5]
    pair, leave = GR.tie_grammar(3)
    score, n_words, words, start = check(model, sym, n, enter, np.full((10, 10), INF), leave)
    iso = D.score(model, sym, n)[0] + enter[None, :] + leave[None, :]
    assert np.array_equal(bits(score), bits(iso.min(axis=1))) and np.array_equal(n_words, np.isfinite(score))
    assert np.array_equal(words[:, 0], D.label_of(iso)) and np.isfinite(score).sum() >= 9
    for e, l in ((np.full(10, INF), leave), (enter, np.full(10, INF))):
        score, n_words, words, start = check(model, sym, n, e, pair, l)
        assert np.isinf(score).all() and not n_words.any() and (words == -1).all() and (start == -1).all()
    ban = np.where(np.eye(10, dtype=bool), INF, np.minimum(pair, 2.0))
    loop = check(model, sym, n, enter, np.minimum(pair, 2.0), leave)
    score, n_words, words, start = check(model, sym, n, enter, ban, leave)
    twice = lambda w, k: sum(int((w[i, 1:k[i]] == w[i, :k[i] - 1]).sum()) for i in range(len(k)))
    assert twice(loop[2], loop[1]) > 0 and twice(words, n_words) == 0 and n_words.max() >= 3


def test_max_words_and_null_arguments():
    model = D.random_models(np.array([1, 2, 1, 3], np.int32), 3, 6, seed=47)
    enter, pair, leave = GR.random_grammar(4, seed=1950, forbid=0.2)
    sym, n = D.random_symbols(12, 20, 6, seed=48, lo=10)
    full = check(model, sym, n, enter, pair, leave)
    top = int(full[1].max())
    assert full[1].min() >= 3 and (full[1] == top - 1).any()
    for mw in (1, top - 1, top):  # 1, and for some utterance exactly n_words and n_words - 1
        got = check(model, sym, n, enter, pair, leave, max_words=mw)
        assert np.array_equal(got[1], full[1]) and np.array_equal(got[2], full[2][:, :mw])
    for name in NAMES:
        got = grammar_raw(model, sym, n, enter, pair, leave, max_words=top - 1, without=(name,))
        assert got[NAMES.index(name)] is None
        same(got, GR.decode(model, sym, n, enter, pair, leave, top - 1))
    same(grammar_raw(model, sym, n, None, pair, leave), GR.decode(model, sym, n, np.zeros(4), pair, leave))
    same(grammar_raw(model, sym, n, enter, pair, None), GR.decode(model, sym, n, enter, pair, np.zeros(4)))
    same(grammar_raw(model, sym, n, None, pair, None), GR.decode(model, sym, n, None, pair, None, form="table"))


def test_two_calls_in_a_graph():
    """Two dsp_dhmm_decode_grammar calls (8 and 32 slots; no allocation, no sync) captured in one single-stream
    graph and replayed twice: the restatement's bits each time."""
    import torch
    from src import _hip
    lib = _hip.lib()
    cases = []
    for Smax, seed in ((5, 2000), (20, 2010)):
        model = R.word_models(7, Smax, 16, seed=seed)
        enter, pair, leave = GR.random_grammar(7, seed=seed + 2, forbid=0.2)
        sym, n = D.random_symbols(9, 50, 16, seed=seed + 1, lo=1)
        want = GR.decode(model, sym, n, enter, pair, leave, 10)
        t = [_dev(a, torch.float64) for a in (model.emit, model.stay, model.adv)] + [_dev(model.n_states, torch.int32)]
        t += [_dev(a, torch.float64) for a in (enter, pair, leave)] + [_dev(sym, torch.int32), _dev(n, torch.int32)]
        outs = [torch.empty(9, dtype=torch.float64, device="cuda"), torch.empty(9, dtype=torch.int32, device="cuda"),
                torch.empty((9, 10), dtype=torch.int32, device="cuda"), torch.empty((9, 10), dtype=torch.int32, device="cuda")]
        nbytes = lib.dsp_dhmm_decode_grammar_workspace_bytes(7, 9, 50, Smax, 16)
        cases.append((Smax, t, outs, torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes, want))

    def call():
        for Smax, t, outs, ws, nbytes, _ in cases:
            rc = lib.dsp_dhmm_decode_grammar(*[_hip.ptr(a) for a in t[:7]], 7, Smax, 16, _hip.ptr(t[7]), _hip.ptr(t[8]), 9, 50,
                                             10, *[_hip.ptr(o) for o in outs], _hip.ptr(ws), nbytes, _hip.stream_handle())
            assert rc == 0

    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        for case in cases:
            for o in case[2]:
                o.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        for case in cases:
            same([o.cpu().numpy() for o in case[2]], case[5])


def test_classifier_decode_with_a_grammar():
    """DiscreteHmmClassifier.decode(grammar=...) on 20 utterances of 2 .. 4 concatenated words against the
    restatement on the tokeniser's own symbols, with the word penalty added through plus; decode(grammar=None)
    is the loop decoder's result, unchanged."""
    from src.models import WordPairGrammar, create_classifier
    from test_gpu_dhmm import pad, word_sequences
    seqs, y = word_sequences(140)
    clf = create_classifier('dhmm', n_states=5, n_codes=16, n_iter=6).fit(seqs, y)
    queries, yq = word_sequences(141)
    rng = np.random.default_rng(142)
    utts, ref, at = [], [], 0
    for _ in range(20):
        k = int(rng.integers(2, 5))
        utts.append(np.concatenate(queries[at:at + k]))
        ref.append(list(np.searchsorted(clf.classes_, yq[at:at + k])))
        at += k
    C = len(clf.classes_)
    penalty = np.array([3.0, 3.5, 4.0])[:C]
    grammar = WordPairGrammar.from_transcripts(ref, C, alpha=0.5)
    labels, starts = clf.decode(utts, word_penalty=penalty, grammar=grammar)
    Xq, nq = pad(utts)
    sym = clf.tokenizer_.transform((Xq - clf.mean_) / clf.std_, nq).cpu().numpy()
    m = clf.model_
    model = D.Model(m.emit, m.stay, m.adv, m.n_states)
    g = grammar.plus(penalty)
    score, n_words, words, start = GR.decode(model, sym, nq, g.enter, g.pair, g.leave)
    assert n_words.min() >= 1
    for i in range(20):
        assert np.array_equal(labels[i], clf.classes_[words[i, :n_words[i]]]) and np.array_equal(starts[i], start[i, :n_words[i]])
    ban = WordPairGrammar.from_allowed(~np.eye(C, dtype=bool))
    banned, _ = clf.decode(utts, word_penalty=penalty, grammar=ban)
    assert all((np.asarray(w)[1:] != np.asarray(w)[:-1]).all() for w in banned)
    one, _ = clf.decode(utts, word_penalty=3.0, max_words=1, grammar=grammar)
    assert all(len(w) == 1 for w in one)
    free, free_starts = clf.decode(utts, word_penalty=penalty)
    _, fn, fw, fs, _ = R.decode(model, sym, nq, penalty)
    for i in range(20):
        assert np.array_equal(free[i], clf.classes_[fw[i, :fn[i]]]) and np.array_equal(free_starts[i], fs[i, :fn[i]])
    with pytest.raises(ValueError):
        clf.decode(utts, grammar=WordPairGrammar.from_allowed(np.ones((C + 1, C + 1), bool)))
