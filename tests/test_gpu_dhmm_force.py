"""GPU tests of csrc/dhmm_force.hip (dsp_dhmm_force_align, dsp_dhmm_force_accumulate) through the bare C ABI,
and of the Python surface on it.  Everything is compared with the numpy restatement of
tests/dhmm_force_reference.py on the raw bits and the raw integers: there is no tolerance and no utterance is
left out.  Every output sits between guard rows, the cost arrays are followed by NaN, and behind each
utterance's length and each transcript's word count the rows hold garbage: -1, K (or C), 2^31 - 1 and INT_MIN."""
import numpy as np
import pytest

import dhmm_decode_reference as R
import dhmm_force_reference as F
import dhmm_reference as D
from device_outputs import Guarded, _dev, bits
from test_gpu_dhmm_decode import _after

pytestmark = pytest.mark.gpu


def _workspace(C, N, T, Wmax, Smax, K):
    import torch
    from src import _hip
    nbytes = _hip.lib().dsp_dhmm_force_workspace_bytes(C, N, T, Wmax, Smax, K)
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes


def force_raw(model, sym, n, trans, L, enter=None, without=()):
    """dsp_dhmm_force_align through the bare C ABI -> (score, seg); an output named in ``without`` is passed as
    NULL and comes back as None."""
    import torch
    from src import _hip
    N, T = sym.shape
    Wmax = trans.shape[1]
    C, Smax, K = model.emit.shape
    keep = [_after(a, torch.float64, np.nan) for a in (model.emit, model.stay, model.adv)]
    keep += [_after(model.n_states, torch.int32, 1 << 20), None if enter is None else _after(enter, torch.float64, np.nan)]
    ts, tn = _after(sym, torch.int32, -5), _after(n, torch.int32, 1 << 20)
    tt, tl = _after(trans, torch.int32, -5), _after(L, torch.int32, 1 << 20)
    outs = {"score": Guarded((N,), torch.float64, -7.0), "seg": Guarded((N, Wmax, Smax), torch.int32, -9)}
    ws, nbytes = _workspace(C, N, T, Wmax, Smax, K)
    rc = _hip.lib().dsp_dhmm_force_align(*[_hip.ptr(t) for t in keep], C, Smax, K, _hip.ptr(ts), _hip.ptr(tn), N, T,
                                         _hip.ptr(tt), _hip.ptr(tl), Wmax,
                                         *[None if name in without else _hip.ptr(o.view) for name, o in outs.items()],
                                         _hip.ptr(ws), nbytes, _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    got = []
    for name, o in outs.items():
        v = o.get()
        if name in without:
            assert (v == o.fill).all(), name
            v = None
        got.append(v)
    return tuple(got)


def accumulate_raw(n_states, K, sym, n, trans, L, seg):
    """dsp_dhmm_force_accumulate through the bare C ABI -> (cnt_emit, cnt, n_valid, valid); the outputs start
    out holding -9, so the call's own zeroing is part of the result."""
    import torch
    from src import _hip
    N, T = sym.shape
    Wmax, Smax = seg.shape[1:]
    C = len(n_states)
    ins = [_after(n_states, torch.int32, 1 << 20), _after(sym, torch.int32, -5), _after(n, torch.int32, 1 << 20),
           _after(trans, torch.int32, -5), _after(L, torch.int32, 1 << 20), _after(seg, torch.int32, 3)]
    outs = [Guarded((C, Smax, K), torch.int32, -9), Guarded((C, Smax), torch.int32, -9), Guarded((C,), torch.int32, -9),
            Guarded((N,), torch.int32, -9)]
    ws, nbytes = _workspace(C, N, T, Wmax, Smax, K)
    rc = _hip.lib().dsp_dhmm_force_accumulate(_hip.ptr(ins[0]), C, Smax, K, _hip.ptr(ins[1]), _hip.ptr(ins[2]), N, T,
                                              _hip.ptr(ins[3]), _hip.ptr(ins[4]), Wmax, _hip.ptr(ins[5]),
                                              *[_hip.ptr(o.view) for o in outs], _hip.ptr(ws), nbytes, _hip.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    return tuple(o.get() for o in outs)


def same(got, want):
    for g, w, name in zip(got, want, ("score", "seg")):
        if g is None:
            continue
        g, w = (bits(v) if v.dtype == np.float64 else v for v in (g, w))
        assert g.shape == w.shape and np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


def same_counts(got, want):
    for g, w, name in zip(got, want, ("cnt_emit", "cnt", "n_valid", "valid")):
        assert g.shape == w.shape and np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


def check(model, sym, n, trans, L, enter=None):
    """Align against the restatement, then accumulate from the device's own seg against the restatement's."""
    want = F.align(model, sym, n, trans, L, enter)
    got = force_raw(model, sym, n, trans, L, enter)
    same(got, want)
    K = model.emit.shape[2]
    counts = F.accumulate(model.n_states, K, sym, n, trans, L, want[1])
    same_counts(accumulate_raw(model.n_states, K, sym, n, trans, L, got[1]), counts)
    assert np.array_equal(counts[3] != 0, np.isfinite(want[0]))
    return want


@pytest.mark.parametrize("C", (1, 2, 10, 64))
def test_model_counts(C):
    model = R.word_models(C, 5, 64, seed=200 + C)
    enter = np.random.default_rng(300 + C).uniform(0, 3, C)
    sym, n = D.random_symbols(20, 40, 64, seed=400 + C, lo=1)
    trans, L = F.random_transcripts(20, 4, C, seed=410 + C)
    score, seg = check(model, sym, n, trans, L, enter)
    assert np.isfinite(score).sum() >= 10 and (np.isfinite(score) & (L >= 3)).sum() >= 3


@pytest.mark.parametrize("Smax", (1, 5, 8, 9, 16, 17, 32))
def test_state_shapes(Smax):
    """The 8-, 16- and 32-slot kernels with Smax at and just past a slot count; mixed n_states with a 0 and an
    Smax + 1 inside transcripts (their tables are NaN and never read); lengths 0, 1, sum S - 1, sum S,
    sum S + 1 of the utterance's own chain, 63 .. 66 and T + 1."""
    rng = np.random.default_rng(500 + Smax)
    states = rng.integers(1, Smax + 1, 10)
    states[[0, 3, 4, 7]] = [Smax, 0, Smax + 1, max(Smax // 2, 1)]
    model = R.word_models(10, Smax, 64, seed=510 + Smax, states=states)
    model.emit[[3, 4]] = model.stay[[3, 4]] = model.adv[[3, 4]] = np.nan  # never read
    N, T = 26, 100
    trans, L = F.random_transcripts(N, 3, 10, seed=520 + Smax)
    trans[np.isin(trans, [3, 4]) & (np.arange(N)[:, None] >= 2)] = 0
    trans[0, 0], trans[1, L[1] - 1] = 3, 4
    chain = np.array([states[trans[u, :L[u]]].sum() for u in range(N)])
    lengths = rng.integers(1, T + 1, N)
    lengths[2:13] = [0, 1, chain[4] - 1, chain[5], chain[6] + 1, 63, 64, 65, 66, T + 1, chain[12]]
    sym, n = D.random_symbols(N, T, 64, seed=530 + Smax, lengths=lengths)
    score, seg = check(model, sym, n, trans, L, rng.uniform(0, 2, 10))
    assert np.isinf(score[[0, 1, 2, 4, 11]]).all() and np.isfinite(score[[5, 6, 12]]).all() and np.isfinite(score).sum() >= 10
    assert (seg[5][seg[5] >= 0] == np.arange(chain[5])).all()  # n = sum S: a frame a state


@pytest.mark.parametrize("K", (1, 2, 256))
def test_alphabets(K):
    model = R.word_models(5, 6, K, seed=600 + K)
    sym, n = D.random_symbols(20, 60, K, seed=610 + K, lo=30)
    sym[3, 0], sym[4, n[4] - 1], sym[5, n[5] // 2], sym[6, 0] = K, -1, 2 ** 31 - 1, -2 ** 31
    trans, L = F.random_transcripts(20, 3, 5, seed=620 + K)
    score, _ = check(model, sym, n, trans, L, np.full(5, 0.5))
    assert np.isinf(score[[3, 4, 5, 6]]).all() and np.isfinite(score).sum() >= 12


@pytest.mark.parametrize("Wmax", (1, 2, 63, 64))
def test_transcript_lengths(Wmax):
    """Word counts 0, 1, Wmax and Wmax + 1, and at Wmax = 64 one word 64 times in a row."""
    model = R.word_models(6, 3, 16, seed=700 + Wmax)
    counts = [0, 1, Wmax, Wmax + 1, Wmax, max(Wmax // 2, 1), Wmax, 1]
    trans, L = F.random_transcripts(8, Wmax, 6, seed=710 + Wmax, counts=counts)
    trans[6] = 2
    sym, n = D.random_symbols(8, 200, 16, seed=720 + Wmax, lengths=[50, 40, 200, 200, 195, 120, 200, 1])
    score, seg = check(model, sym, n, trans, L, np.full(6, 0.25))
    assert np.isinf(score[[0, 3]]).all() and np.isfinite(score[[1, 2, 4, 5, 6]]).all()
    assert (seg[6, :, 0] >= 0).all() and (np.diff(seg[6, :, 0]) >= model.n_states[2]).all()


def test_longest_chains():
    """T = 1024: 64 positions of 16 states, the largest chain that fits 1024 frames, at 1024 frames (a frame a
    state) and with mixed n_states; 32 positions of 32 states."""
    model = R.word_models(8, 16, 32, seed=800, states=[16, 16, 9, 16, 12, 16, 16, 16])
    trans, L = F.random_transcripts(2, 64, 8, seed=801, counts=[64, 64])
    trans[0][np.isin(trans[0], [2, 4])] = 0
    sym, n = D.random_symbols(2, 1024, 32, seed=802, lengths=[1024, 1024])
    score, seg = check(model, sym, n, trans, L, np.full(8, 1.0))
    assert np.isfinite(score).all() and np.array_equal(seg[0].reshape(-1), np.arange(1024))
    model = R.word_models(8, 32, 32, seed=810, states=[32] * 8)
    trans, L = F.random_transcripts(2, 32, 8, seed=811, counts=[32, 31])
    score, seg = check(model, sym, n, trans, L, np.full(8, 1.0))
    assert np.isfinite(score).all() and np.array_equal(seg[0].reshape(-1), np.arange(1024))


@pytest.mark.parametrize("N, T", ((1, 12), (2, 12), (65, 12), (1030, 1024)))
def test_utterance_counts(N, T):
    """At T = 1024 the direction words let 1024 waves be resident: with N = 1030 a wave takes a second utterance
    (short rows: at most 8 frames)."""
    model = R.word_models(10, 3, 16, seed=900)
    sym, n = D.random_symbols(N, T, 16, seed=901 + N, lengths=np.random.default_rng(902 + N).integers(0, 9, N))
    trans, L = F.random_transcripts(N, 2, 10, seed=903 + N)
    score, _ = check(model, sym, n, trans, L, np.full(10, 0.25))
    assert np.isfinite(score).sum() >= N // 3


@pytest.mark.parametrize("seed", (1, 2))
def test_tie_rule(seed):
    """The dyadic tie corpus: the strict < of the cells decides score and path."""
    model, enter, sym, n, trans, L = F.tie_corpus(seed)
    stats = [0, 0]
    F.align(model, sym, n, trans, L, enter, stats=stats)
    assert stats[1] / stats[0] >= 0.04, stats
    check(model, sym, n, trans, L, enter)


def test_entry_costs_and_null_outputs():
    model = R.word_models(4, 6, 8, seed=1000, states=[4, 6, 5, 2])
    sym, n = D.random_symbols(12, 40, 8, seed=1001, lo=20)
    trans, L = F.random_transcripts(12, 3, 4, seed=1002)
    same(force_raw(model, sym, n, trans, L, None), F.align(model, sym, n, trans, L, np.zeros(4)))
    score, seg = check(model, sym, n, trans, L, np.full(4, np.inf))
    assert np.isinf(score).all() and (seg == -1).all()
    one = np.array([0.5, np.inf, 0.0, 1.0])
    score, _ = check(model, sym, n, trans, L, one)
    uses = np.array([(trans[u, :L[u]] == 1).any() for u in range(12)])
    assert np.isinf(score[uses]).all() and np.isfinite(score[~uses]).all() and 3 <= uses.sum() <= 10
    want = F.align(model, sym, n, trans, L, one)
    for name in ("score", "seg"):
        got = force_raw(model, sym, n, trans, L, one, without=(name,))
        assert got[("score", "seg").index(name)] is None
        same(got, want)


def test_against_the_isolated_alignment_and_the_decoder():
    """The consequences of the definition on the device: (a) L = 1 and enter = 0 give dsp_dhmm_align's score
    and seg row; (b) forcing dsp_dhmm_decode's own words gives dsp_dhmm_decode's score, and its word starts on
    this non-dyadic corpus; another transcript scores no less."""
    from src.pipeline import DhmmModelSet, dhmm_align, dhmm_decode
    model = D.random_models(np.array([4, 5, 1, 6], np.int32), 6, 11, seed=41)
    dm = DhmmModelSet.from_arrays(model.emit, model.stay, model.adv, model.n_states)
    sym, n = D.random_symbols(40, 12, 11, seed=42, lo=1)
    word = np.arange(40, dtype=np.int32) % 4
    score, seg = force_raw(model, sym, n, word[:, None], np.ones(40, np.int32), np.zeros(4))
    iso, iso_seg, _, members = (t.cpu().numpy() for t in dhmm_align(dm, sym, n, assign=word))
    assert np.array_equal(bits(score[members]), bits(iso)) and np.array_equal(seg[members, 0], iso_seg)
    assert np.isfinite(score).sum() >= 25 and np.isinf(score).sum() >= 3

    model = D.random_models(np.array([2, 3, 1, 4], np.int32), 4, 6, seed=43)
    dm = DhmmModelSet.from_arrays(model.emit, model.stay, model.adv, model.n_states)
    enter = np.array([0.5, 0.25, 1.5, 0.0])
    sym, n = D.random_symbols(30, 25, 6, seed=44, lo=8)
    dec, n_words, words, start, _ = (t.cpu().numpy() for t in dhmm_decode(dm, sym, n, enter=enter))
    Wmax = int(n_words.max())
    score, seg = force_raw(model, sym, n, words[:, :Wmax], n_words, enter)
    assert np.array_equal(bits(score), bits(dec)) and np.array_equal(seg[:, :, 0], start[:, :Wmax])
    other, L = F.random_transcripts(30, Wmax, 4, seed=45)
    assert (force_raw(model, sym, n, other, L, enter)[0] >= dec).all()


def test_accumulate_skips_damaged_rows():
    model = R.word_models(5, 4, 7, seed=70, states=[2, 4, 1, 3, 4])
    sym, n = D.random_symbols(30, 40, 7, seed=71, lo=10)
    trans, L = F.random_transcripts(30, 4, 5, seed=72)
    seg = force_raw(model, sym, n, trans, L, np.full(5, 0.5))[1].copy()
    good = np.flatnonzero((seg[:, 0, 0] == 0) & (L >= 2) & (seg == -1).any(axis=(1, 2)))[:5]
    assert len(good) == 5
    u0, u1, u2, u3, u4 = good
    last = lambda u, i: model.n_states[trans[u, i]] - 1
    seg[u0, 0, 0] = 1                                # not starting at 0
    seg[u1, 1, 0] = seg[u1, 0, last(u1, 0)]          # a repeated frame
    seg[u2, L[u2] - 1, last(u2, L[u2] - 1)] = n[u2]  # a last frame >= n
    i, s = np.argwhere(seg[u3] == -1)[0]
    seg[u3, i, s] = n[u3] - 1                        # an entry where the definition says -1
    seg[u4, 1, 0] = -1                               # a stray -1 inside the chain
    sym[7, 3], n[8] = 7, 41                          # a symbol outside the alphabet, a bad length
    want = F.accumulate(model.n_states, 7, sym, n, trans, L, seg)
    assert not want[3][list(good) + [7, 8]].any() and want[3].sum() >= 12
    same_counts(accumulate_raw(model.n_states, 7, sym, n, trans, L, seg), want)
    junk = np.random.default_rng(73).integers(-3, 45, seg.shape).astype(np.int32)  # no row is well formed
    want = F.accumulate(model.n_states, 7, sym, n, trans, L, junk)
    assert not want[3].any() and not want[0].any()
    same_counts(accumulate_raw(model.n_states, 7, sym, n, trans, L, junk), want)


def test_two_calls_in_a_graph():
    """Two dsp_dhmm_force_align calls (8 and 32 slots; no allocation, no sync) captured in one single-stream
    graph and replayed twice: the restatement's bits each time."""
    import torch
    from src import _hip
    lib = _hip.lib()
    cases = []
    for Smax, seed in ((5, 1100), (20, 1110)):
        model = R.word_models(7, Smax, 16, seed=seed)
        enter = np.full(7, 0.5)
        sym, n = D.random_symbols(9, 90, 16, seed=seed + 1, lo=30)
        trans, L = F.random_transcripts(9, 3, 7, seed=seed + 2)
        want = F.align(model, sym, n, trans, L, enter)
        t = [_dev(a, torch.float64) for a in (model.emit, model.stay, model.adv)] + [_dev(model.n_states, torch.int32)]
        t += [_dev(enter, torch.float64), _dev(sym, torch.int32), _dev(n, torch.int32), _dev(trans, torch.int32),
              _dev(L, torch.int32)]
        outs = [torch.empty(9, dtype=torch.float64, device="cuda"), torch.empty((9, 3, Smax), dtype=torch.int32, device="cuda")]
        ws, nbytes = _workspace(7, 9, 90, 3, Smax, 16)
        cases.append((Smax, t, outs, ws, nbytes, want))

    def call():
        for Smax, t, outs, ws, nbytes, _ in cases:
            rc = lib.dsp_dhmm_force_align(*[_hip.ptr(a) for a in t[:5]], 7, Smax, 16, _hip.ptr(t[5]), _hip.ptr(t[6]), 9, 90,
                                          _hip.ptr(t[7]), _hip.ptr(t[8]), 3, *[_hip.ptr(o) for o in outs], _hip.ptr(ws),
                                          nbytes, _hip.stream_handle())
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


def test_classifier_align_and_fit_connected():
    """DiscreteHmmClassifier.fit_connected on 20 utterances of 2 .. 4 concatenated words and their transcripts
    against the restatement on the tokeniser's own symbols: model_ bit for bit, totals_ equal; then ``align``
    against the restatement under that model."""
    from src.models import create_classifier
    from test_gpu_dhmm import pad, word_sequences
    queries, yq = word_sequences(141)
    rng = np.random.default_rng(142)
    utts, ref, at = [], [], 0
    for _ in range(20):
        k = int(rng.integers(2, 5))
        utts.append(np.concatenate(queries[at:at + k]))
        ref.append(list(yq[at:at + k]))
        at += k
    penalty = np.array([3.0, 3.5, 4.0])
    clf = create_classifier('dhmm', n_states=5, n_codes=16, n_iter=4, scoring='forward')
    assert clf.fit_connected(utts, ref, word_penalty=penalty) is clf
    assert np.array_equal(clf.classes_, [2, 7, 12]) and 1 <= clf.n_iter_ <= 4
    Xq, nq = pad(utts)
    sym = clf.tokenizer_.transform((Xq - clf.mean_) / clf.std_, nq).cpu().numpy()
    L = np.array([len(r) for r in ref], np.int32)
    trans = np.full((20, 4), -1, np.int32)
    for i, r in enumerate(ref):
        trans[i, :len(r)] = np.searchsorted(clf.classes_, r)
    model, totals, _ = F.fit_connected(sym, nq, trans, L, np.full(3, 5), 16, n_iter=4, enter=penalty)
    for f in ("emit", "stay", "adv"):
        assert np.array_equal(bits(getattr(clf.model_, f)), bits(getattr(model, f))), f
    assert np.array_equal(bits(clf.totals_), bits(totals)) and clf.totals_.shape == (clf.n_iter_,)
    assert clf.prob_.pemit.shape == clf.model_.emit.shape == (3, 5, 16)
    starts, scores = clf.align(utts, ref, word_penalty=penalty)
    want, seg = F.align(model, sym, nq, trans, L, penalty)
    assert np.array_equal(bits(scores), bits(want)) and np.isfinite(want).all()
    for i in range(20):
        assert np.array_equal(starts[i], seg[i, :L[i], 0]) and starts[i][0] == 0
    starts, scores = clf.align(utts[:2], [ref[0], [2] * 60], word_penalty=penalty)  # 300 states: more than the frames
    assert len(starts[0]) == L[0] and len(starts[1]) == 0 and np.isinf(scores[1])
    with pytest.raises(ValueError):
        clf.align(utts[:1], [[2, 3]])
