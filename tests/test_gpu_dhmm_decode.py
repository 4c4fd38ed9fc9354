"""GPU tests of csrc/dhmm_decode.hip (dsp_dhmm_decode) through the bare C ABI, and of the Python surface on
it.  Everything is compared with the numpy restatement of tests/dhmm_decode_reference.py on the raw bits
and the raw integers: there is no tolerance and no utterance is left out.  Every output sits between guard
rows, and behind each utterance's length the symbol rows hold garbage: -1, K, 2^31 - 1 and INT_MIN."""
import numpy as np
import pytest

import dhmm_decode_reference as R
import dhmm_reference as D
from device_outputs import Guarded, _dev, bits

pytestmark = pytest.mark.gpu

NAMES = ("score", "n_words", "words", "start", "cum")


def _after(x, dtype, fill):
    """An input followed by 64 entries of fill (NaN for costs): a read past its end would show in a result."""
    import torch
    x = np.asarray(x, np.float64 if dtype == torch.float64 else np.int32).reshape(-1)
    return _dev(np.concatenate([x, np.full(64, fill, x.dtype)]), dtype)


def decode_raw(model, sym, n, enter=None, max_words=None, without=()):
    """dsp_dhmm_decode through the bare C ABI -> (score, n_words, words, start, cum); the outputs named in
    ``without`` are passed as NULL and come back as None."""
    import torch
    from src import _hip
    N, T = sym.shape
    C, Smax, K = model.emit.shape
    mw = T if max_words is None else max_words
    keep = [_after(a, torch.float64, np.nan) for a in (model.emit, model.stay, model.adv)]
    keep += [_after(model.n_states, torch.int32, 1 << 20), None if enter is None else _after(enter, torch.float64, np.nan)]
    ts, tn = _after(sym, torch.int32, -5), _dev(np.asarray(n, np.int32), torch.int32)
    outs = [Guarded((N,), torch.float64, -7.0), Guarded((N,), torch.int32, -9), Guarded((N, mw), torch.int32, -9),
            Guarded((N, mw), torch.int32, -9), Guarded((N, mw), torch.float64, -7.0)]
    nbytes = _hip.lib().dsp_dhmm_decode_workspace_bytes(C, N, T, Smax, K)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = _hip.lib().dsp_dhmm_decode(*[_hip.ptr(t) for t in keep], C, Smax, K, _hip.ptr(ts), _hip.ptr(tn), N, T, mw,
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


def check(model, sym, n, enter=None, max_words=None):
    want = R.decode(model, sym, n, enter, max_words)
    same(decode_raw(model, sym, n, enter, max_words), want)
    return want


@pytest.mark.parametrize("C", (1, 2, 3, 10, 63, 64))
def test_model_counts(C):
    model = R.word_models(C, 5, 64, seed=200 + C)
    enter = np.random.default_rng(300 + C).uniform(0, 3, C)
    sym, n = D.random_symbols(20, 40, 64, seed=400 + C, lo=1)
    score, n_words = check(model, sym, n, enter)[:2]
    assert np.isfinite(score).sum() >= 15 and n_words.max() >= 2


EDGE = lambda S: [0, 1, 2, max(S - 1, 1), S, 2 * S, 63, 64, 65, 66]


@pytest.mark.parametrize("Smax", (1, 5, 8, 16, 17, 32))
def test_state_shapes(Smax):
    """The 8-, 16- and 32-slot kernels with Smax at and just past a slot count; mixed n_states with a 0 and
    an Smax + 1 among them; lengths 0, 1, 2, S - 1, S, 2 S, 63 .. 65 and T + 1."""
    rng = np.random.default_rng(500 + Smax)
    states = rng.integers(1, Smax + 1, 10)
    states[[0, 3, 4, 7]] = [Smax, 0, Smax + 1, max(Smax // 2, 1)]
    model = R.word_models(10, Smax, 64, seed=510 + Smax, states=states)
    model.emit[[3, 4]] = np.nan  # never read
    lengths = np.concatenate([EDGE(Smax), rng.integers(1, 66, 12)])
    sym, n = D.random_symbols(len(lengths), 65, 64, seed=520 + Smax, lengths=lengths)
    score, n_words, words = check(model, sym, n, rng.uniform(0, 2, 10))[:3]
    assert np.isinf(score[[0, 9]]).all() and np.isfinite(score).sum() >= 15 and not np.isin(words, [3, 4]).any()
    assert n_words.max() >= (2 if Smax > 1 else 30)


@pytest.mark.parametrize("K", (1, 2, 256))
def test_alphabets(K):
    model = R.word_models(5, 6, K, seed=600 + K)
    sym, n = D.random_symbols(20, 30, K, seed=610 + K, lo=1)
    sym[3, 0], sym[4, n[4] - 1], sym[5, n[5] // 2], sym[6, 0] = K, -1, 2 ** 31 - 1, -2 ** 31
    score = check(model, sym, n, np.full(5, 0.5))[0]
    assert np.isinf(score[[3, 4, 5, 6]]).all() and np.isfinite(score).sum() >= 12


def test_longest_utterance():
    """One utterance at T = 1024 with C = 64 and Smax = 32 (32 slots, the transitions in LDS), and one frame
    short of it."""
    model = R.word_models(64, 32, 64, seed=700)
    sym, n = D.random_symbols(2, 1024, 64, seed=701, lengths=[1024, 1023])
    score, n_words = check(model, sym, n, np.full(64, 1.0))[:2]
    assert np.isfinite(score).all() and n_words.min() >= 5


@pytest.mark.parametrize("N", (1, 2, 65, 300, 8300))
def test_utterance_counts(N):
    """N = 8300 is more than the persistent grid of 8192 waves holds: a wave takes a second utterance."""
    model = R.word_models(10, 5, 16, seed=800)
    sym, n = D.random_symbols(N, 12 if N < 1000 else 6, 16, seed=801 + N, lo=0)
    score = check(model, sym, n, np.full(10, 0.25), max_words=6)[0]
    assert np.isfinite(score).sum() >= N // 3


@pytest.mark.parametrize("seed", (1, 2))
def test_tie_rule(seed):
    """The dyadic tie corpus: the strict < of the cells and the smallest-index rule of the exit decide."""
    model, enter, sym, n = R.tie_corpus(seed)
    stats = [0, 0, 0, 0]
    want = R.decode(model, sym, n, enter, stats=stats)
    assert stats[1] / stats[0] >= 0.08 and stats[3] / stats[2] >= 0.10, stats
    same(decode_raw(model, sym, n, enter), want)


def test_duplicated_models():
    model = D.random_models(np.array([2, 3, 2, 3, 1], np.int32), 3, 6, seed=45)
    for a in (model.emit, model.stay, model.adv):
        a[2], a[3] = a[0], a[1]
    sym, n = D.random_symbols(30, 25, 6, seed=46, lo=5)
    words = check(model, sym, n, np.array([0.5, 0.25, 0.5, 0.25, 1.0]))[2]
    assert np.isin(words, [0, 1]).sum() > 40 and not np.isin(words, [2, 3]).any()


def test_nothing_to_decode():
    """enter all +inf; utterances shorter than every model; a model set whose every exit is closed."""
    model = R.word_models(4, 6, 8, seed=900, states=[4, 6, 5, 4])
    sym, n = D.random_symbols(12, 20, 8, seed=901, lengths=[1, 2, 3, 4, 5, 8, 12, 20, 3, 2, 1, 16])
    score, n_words, words, start, cum = check(model, sym, n, np.full(4, np.inf))
    assert np.isinf(score).all() and not n_words.any() and (words == -1).all() and np.isinf(cum).all()
    score, n_words = check(model, sym, n, np.zeros(4))[:2]
    assert np.isinf(score[n < 4]).all() and not n_words[n < 4].any() and np.isfinite(score[n >= 4]).all()
    model.emit[:, 3:, :] = np.inf  # no model reaches its last state
    assert np.isinf(check(model, sym, n, np.zeros(4))[0]).all()


def test_max_words_and_null_outputs():
    model = D.random_models(np.array([1, 2, 1, 3], np.int32), 3, 6, seed=47)
    enter = np.array([0.5, 0.0, 1.0, 0.0])
    sym, n = D.random_symbols(12, 20, 6, seed=48, lo=10)
    full = check(model, sym, n, enter)
    top = int(full[1].max())
    assert full[1].min() >= 3 and (full[1] == top - 1).any()
    for mw in (1, top - 1, top):  # 1, and for some utterance exactly n_words and n_words - 1
        got = check(model, sym, n, enter, max_words=mw)
        assert np.array_equal(got[1], full[1]) and np.array_equal(got[2], full[2][:, :mw])
    for name in NAMES:
        got = decode_raw(model, sym, n, enter, max_words=top - 1, without=(name,))
        assert got[NAMES.index(name)] is None
        same(got, R.decode(model, sym, n, enter, top - 1))
    same(decode_raw(model, sym, n, None), R.decode(model, sym, n, np.zeros(4)))


def test_against_the_isolated_word_scores():
    """The consequences of the definition, against dsp_dhmm_score on the device: with enter = 0.0 and
    n < 2 min S the score is the smallest isolated score and words[0] its label; with enter[words[0]] = 0.0
    cum[0] is the isolated score of the prefix sym[0 : start[1]] under words[0]."""
    from src.pipeline import DhmmModelSet, dhmm_score
    model = D.random_models(np.array([4, 5, 4, 6], np.int32), 6, 11, seed=41)
    dm = DhmmModelSet.from_arrays(model.emit, model.stay, model.adv, model.n_states)
    sym, n = D.random_symbols(30, 7, 11, seed=42, lo=1)
    score, n_words, words, start, cum = decode_raw(model, sym, n, np.zeros(4))
    iso, label = (t.cpu().numpy() for t in dhmm_score(dm, sym, n, with_labels=True))
    assert np.array_equal(bits(score), bits(iso.min(axis=1))) and np.array_equal(words[:, 0], label)
    assert np.isfinite(score).sum() >= 10 and np.array_equal(n_words, np.isfinite(score))
    sym, n = D.random_symbols(30, 25, 11, seed=44, lo=12)
    score, n_words, words, start, cum = decode_raw(model, sym, n, np.zeros(4))
    assert (n_words >= 1).all() and (n_words >= 2).sum() >= 15
    iso = dhmm_score(dm, sym, np.where(n_words >= 2, start[:, 1], n))[0].cpu().numpy()
    assert np.array_equal(bits(cum[:, 0]), bits(iso[np.arange(30), words[:, 0]]))


def test_two_calls_in_a_graph():
    """Two dsp_dhmm_decode calls (8 and 32 slots; no allocation, no sync) captured in one single-stream graph
    and replayed twice: the restatement's bits each time."""
    import torch
    from src import _hip
    lib = _hip.lib()
    cases = []
    for Smax, seed in ((5, 1000), (20, 1010)):
        model = R.word_models(7, Smax, 16, seed=seed)
        enter = np.full(7, 0.5)
        sym, n = D.random_symbols(9, 50, 16, seed=seed + 1, lo=1)
        want = R.decode(model, sym, n, enter, 10)
        t = [_dev(a, torch.float64) for a in (model.emit, model.stay, model.adv)] + [_dev(model.n_states, torch.int32)]
        t += [_dev(enter, torch.float64), _dev(sym, torch.int32), _dev(n, torch.int32)]
        outs = [torch.empty(9, dtype=torch.float64, device="cuda"), torch.empty(9, dtype=torch.int32, device="cuda"),
                torch.empty((9, 10), dtype=torch.int32, device="cuda"), torch.empty((9, 10), dtype=torch.int32, device="cuda"),
                torch.empty((9, 10), dtype=torch.float64, device="cuda")]
        nbytes = lib.dsp_dhmm_decode_workspace_bytes(7, 9, 50, Smax, 16)
        cases.append((Smax, t, outs, torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes, want))

    def call():
        for Smax, t, outs, ws, nbytes, _ in cases:
            rc = lib.dsp_dhmm_decode(*[_hip.ptr(a) for a in t[:5]], 7, Smax, 16, _hip.ptr(t[5]), _hip.ptr(t[6]), 9, 50, 10,
                                     *[_hip.ptr(o) for o in outs], _hip.ptr(ws), nbytes, _hip.stream_handle())
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


def test_classifier_decode():
    """DiscreteHmmClassifier.decode on 20 utterances of 2 .. 4 concatenated words against the restatement on
    the tokeniser's own symbols; the words come out mostly right on this easy corpus."""
    from src.models import create_classifier, word_error_rate
    from test_gpu_dhmm import pad, word_sequences
    seqs, y = word_sequences(140)
    clf = create_classifier('dhmm', n_states=5, n_codes=16, n_iter=6).fit(seqs, y)
    queries, yq = word_sequences(141)
    rng = np.random.default_rng(142)
    utts, ref, at = [], [], 0
    for _ in range(20):
        k = int(rng.integers(2, 5))
        utts.append(np.concatenate(queries[at:at + k]))
        ref.append(list(yq[at:at + k]))
        at += k
    penalty = np.array([3.0, 3.5, 4.0])
    labels, starts = clf.decode(utts, word_penalty=penalty)
    Xq, nq = pad(utts)
    sym = clf.tokenizer_.transform((Xq - clf.mean_) / clf.std_, nq).cpu().numpy()
    m = clf.model_
    score, n_words, words, start, cum = R.decode(D.Model(m.emit, m.stay, m.adv, m.n_states), sym, nq, penalty)
    for i in range(20):
        assert np.array_equal(labels[i], clf.classes_[words[i, :n_words[i]]]) and np.array_equal(starts[i], start[i, :n_words[i]])
    assert word_error_rate(ref, labels) < 0.5
    one, _ = clf.decode(utts, word_penalty=3.0, max_words=1)
    assert all(len(w) == 1 for w in one)
    with pytest.raises(ValueError):
        clf.decode(utts, max_words=0)
