"""CPU tests of the discrete-HMM definition (tests/dhmm_reference.py) and of the host side on it: the two
forms of the restatement agree bit for bit, the path is the brute force's over all segmentations with the
tie rule, accumulate and the model build on hand-worked cases, and the loaded library's argument checks."""
import ctypes
import itertools

import numpy as np
import pytest

import dhmm_reference as D


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def all_pairs(C, N):
    return np.arange(C + 1) * N, np.tile(np.arange(N), C)


def dyadic_corpus():
    """9 models of 1 .. 6 states over K = 3 symbols, costs multiples of 1/8, 60 rows of up to 24 symbols."""
    model = D.dyadic_models([1, 2, 3, 4, 5, 6, 3, 2, 4], 6, 3, seed=12)
    sym, n = D.random_symbols(60, 24, 3, seed=13)
    return model, sym, n


@pytest.mark.parametrize("corpus", ("random", "dyadic"))
def test_the_two_forms_agree(corpus):
    if corpus == "dyadic":
        model, sym, n = dyadic_corpus()
    else:
        model = D.random_models([1, 2, 5, 7, 3], 7, 17, seed=1)
        model.emit[1, 0, 3] = model.emit[2, 2, :] = np.inf  # a +inf emission and an all-+inf row
        sym, n = D.random_symbols(40, 20, 17, seed=2)
        sym[3, 0], sym[4, n[4] - 1], sym[5, n[5] // 2] = 17, -1, 2 ** 31 - 1  # symbols outside the alphabet
    start, members = all_pairs(len(model.n_states), len(sym))
    st, gt = D.align(model, sym, n, start, members, "table")
    sr, gr = D.align(model, sym, n, start, members, "rows")
    assert np.array_equal(bits(st), bits(sr)) and np.array_equal(gt, gr)
    assert np.isfinite(st).sum() > 100 and np.isinf(st).any() and not np.isnan(st).any()
    assert (gt[np.isinf(st)] == -1).all()
    full, label = D.score(model, sym, n, "table")
    assert np.array_equal(bits(full), bits(D.score(model, sym, n)[0]))
    assert np.array_equal(bits(full.T.reshape(-1)), bits(st))
    if corpus == "random":
        assert np.isinf(full[[3, 4, 5]]).all() and (label[[3, 4, 5]] == -1).all()
        assert np.isinf(full[n >= 5, 2]).all()  # the all-+inf row of model 2


def test_dyadic_corpus_ties():
    """A condition on the input: at least a tenth of the decided cells of the dyadic corpus have a == b."""
    model, sym, n = dyadic_corpus()
    ties = [0, 0]
    D.align(model, sym, n, *all_pairs(len(model.n_states), len(sym)), ties=ties)
    assert ties[0] > 5000 and ties[1] / ties[0] >= 0.10, ties


def brute_force(sym, emit, stay, adv):
    """(cost, seg) over every segmentation of the n symbols into S non-empty runs: the smallest cost (dyadic
    values: every sum is exact), and among equal costs the path the tie rule keeps -- walking back, a tie
    stays, so the last state starts as early as it can, then the one before it, and so on."""
    n, S = len(sym), len(stay)
    best = None
    for cut in itertools.combinations(range(1, n), S - 1):
        b = (0,) + cut + (n,)
        cost = 0.0
        for s in range(S):
            cost += sum(emit[s, sym[t]] for t in range(b[s], b[s + 1])) + (b[s + 1] - b[s] - 1) * stay[s]
            cost += adv[s - 1] if s else 0.0
        key = (cost,) + tuple(reversed(b[1:S]))
        if best is None or key < best[0]:
            best = key, list(b[:S])
    return (np.inf, None) if best is None else (best[0][0], best[1])


def test_the_path_is_the_brute_force_minimum():
    model = D.dyadic_models([1, 2, 3, 4, 4, 3, 2, 4], 4, 3, seed=21)
    sym, n = D.random_symbols(50, 8, 3, seed=22)
    tied = 0
    for c in range(len(model.n_states)):
        m = model.one(c)
        for i in range(len(sym)):
            got = D.viterbi_table(sym[i, :n[i]], *m)
            want = brute_force(sym[i, :n[i]], *m)
            assert got[0] == want[0] and got[1] == want[1], (c, i, got, want)
            tied += want[1] is not None
    assert tied > 150


def test_accumulate_by_hand():
    """Two models (S = 2, K = 3 and an n_states of 0) and four members: a clean one, one whose seg row is
    not increasing, one with a symbol outside the alphabet in its last frame, and another clean one."""
    sym = np.array([[0, 1, 1, 2, -1], [2, 2, 0, 7, 7], [1, 1, 3, 9, 9], [2, 0, 0, 0, 1]], np.int32)
    n = np.array([4, 3, 3, 5], np.int32)
    seg = np.array([[0, 2], [0, 0], [0, 1], [0, 1], [0, 1]], np.int32)
    start, members = [0, 4, 5], [0, 1, 2, 3, 0]
    score = np.array([1.5, 100.0, 200.0, 0.1, 7.0])
    cnt_emit, cnt, n_valid, total = D.accumulate([2, 0], 3, sym, n, start, members, seg, score)
    assert cnt_emit[0].tolist() == [[1, 1, 1], [3, 2, 1]] and cnt[0].tolist() == [3, 6]
    assert n_valid.tolist() == [2, 0] and total.tolist() == [1.5 + 0.1, 0.0]
    assert not cnt_emit[1].any() and not cnt[1].any()
    swapped = D.accumulate([2, 0], 3, sym, n, start, [3, 1, 2, 0, 0], seg[[3, 1, 2, 0, 4]], score[[3, 1, 2, 0, 4]])
    assert np.array_equal(swapped[0], cnt_emit) and swapped[3][0] == 0.1 + 1.5


def test_model_build():
    from src.pipeline import DhmmModelSet
    cnt_emit = np.array([[[1, 1, 1], [3, 3, 1]], [[0, 0, 0], [0, 0, 0]], [[5, 0, 0], [0, 0, 0]]])
    cnt = np.array([[3, 7], [0, 0], [5, 0]])
    n_valid, states = np.array([2, 0, 5]), np.array([2, 2, 1])
    want = D.build_model(cnt_emit, cnt, n_valid, states, 0.5, 0.25)
    got = DhmmModelSet(cnt_emit, cnt, n_valid, states, 0.5, 0.25)
    for name in ("emit", "stay", "adv"):
        assert np.array_equal(bits(getattr(got, name)), bits(getattr(want, name))), name
    assert got.emit[0, 1, 2] == -np.log((1 + 0.5) / (7 + 0.5 * 3)) and got.emit[0, 0, 0] == -np.log(1.5 / 4.5)
    assert (got.emit[1] == -np.log(0.5 / 1.5)).all()  # nothing counted: uniform by itself
    assert not got.emit[2, 1].any() and not got.stay[2, 1] and got.emit[2, 0, 1] == -np.log(0.5 / 6.5)
    assert got.stay[0, 0] == -np.log(1 / 3) and got.adv[0, 1] == -np.log(1 - 5 / 7)
    assert got.stay[1, 0] == -np.log(0.5) and got.stay[2, 0] == -np.log(0.25)  # (5 - 5) / 5 = 0 -> the floor
    again = DhmmModelSet(cnt_emit, cnt, n_valid, states, 0.5, 0.25, prev=DhmmModelSet.from_arrays(
        want.emit, want.stay + 1.0, want.adv + 2.0, states))
    assert np.array_equal(bits(again.stay[1]), bits(want.stay[1] + 1.0)) and np.array_equal(bits(again.stay[0]), bits(want.stay[0]))
    prev = D.Model(want.emit, want.stay + 1.0, want.adv + 2.0, states)
    assert np.array_equal(bits(again.adv), bits(D.build_model(cnt_emit, cnt, n_valid, states, 0.5, 0.25, prev=prev).adv))
    hand = DhmmModelSet.from_arrays(np.full((1, 2, 4), np.inf), np.zeros((1, 2)), np.ones((1, 2)), [2])
    assert hand.shape == (1, 2, 4) and np.isinf(hand.emit).all()
    for bad in (dict(alpha=0.0), dict(alpha=-1.0), dict(trans_floor=0.5)):
        with pytest.raises(ValueError):
            DhmmModelSet(cnt_emit, cnt, n_valid, states, **bad)
    with pytest.raises(ValueError):
        DhmmModelSet.from_arrays(np.full((1, 2, 4), -np.inf), np.zeros((1, 2)), np.ones((1, 2)), [2])
    with pytest.raises(ValueError):
        DhmmModelSet.from_arrays(np.zeros((1, 2, 257)), np.zeros((1, 2)), np.ones((1, 2)), [2])


def test_create_classifier_validates_without_a_device():
    from src.models import DiscreteHmmClassifier, SequenceClassifier, create_classifier
    from src.pipeline import DHMM_MAX_SYMBOLS, VqTokenizer
    clf = create_classifier('dhmm')
    assert isinstance(clf, DiscreteHmmClassifier) and isinstance(clf, SequenceClassifier) and DHMM_MAX_SYMBOLS == 256
    assert (clf.n_states, clf.n_codes, clf.n_iter, clf.alpha, clf.trans_floor, clf.vq_iter, clf.eps, clf.normalize) == \
        (5, 64, 10, 0.5, 1e-3, 10, 0.01, True)
    for bad in (dict(n_states=0), dict(n_states=33), dict(n_codes=48), dict(n_codes=512), dict(alpha=0.0), dict(n_iter=-1),
                dict(trans_floor=0.5), dict(vq_iter=0), dict(eps=0.0)):
        with pytest.raises(ValueError):
            create_classifier('dhmm', **bad)
    assert VqTokenizer(8).n_codes == 8
    with pytest.raises(NotImplementedError):
        clf.kneighbors([np.zeros((3, 2))])


def test_abi_argument_checks():
    """The plan's bounds and the NULL checks, answered on the host before any launch."""
    from src import _hip
    lib = _hip.load_library()
    wb = lib.dsp_dhmm_workspace_bytes
    assert wb(10, 100, 100, 64, 5, 64) > 0 and wb(10, 100, 0, 1024, 32, 256) > 0 and wb(0, 0, 0, 1, 1, 1) > 0
    for args in ((10, 100, 100, 1025, 5, 64), (10, 100, 100, 0, 5, 64), (10, 100, 100, 64, 33, 64), (10, 100, 100, 64, 0, 64),
                 (10, 100, 100, 64, 5, 257), (10, 100, 100, 64, 5, 0), (-1, 100, 100, 64, 5, 64), (10, -1, 100, 64, 5, 64),
                 (10, 100, -1, 64, 5, 64), ((1 << 20) + 1, 100, 100, 64, 5, 64)):
        assert wb(*args) == 0, args
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    model = (p, p, p, p, 3, 5, 64)  # emit, stay, adv, n_states, C, Smax, K
    big = 1 << 30
    assert lib.dsp_dhmm_score(p, p, p, p, 3, 5, 257, p, p, 4, 64, p, p, p, big, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_dhmm_score(p, p, p, p, 3, 5, 0, p, p, 4, 64, p, p, p, big, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_dhmm_score(p, p, p, p, 3, 33, 64, p, p, 4, 64, p, p, p, big, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_dhmm_score(*model, p, p, 4, 1025, p, p, p, big, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_dhmm_score(None, p, p, p, 3, 5, 64, p, p, 4, 64, p, p, p, big, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_dhmm_score(*model, None, p, 4, 64, p, p, p, big, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_dhmm_score(*model, p, p, 4, 64, p, p, None, 0, None) == _hip.DSP_ERR_WORKSPACE
    assert lib.dsp_dhmm_score(*model, p, p, 4, 64, p, p, p, 8, None) == _hip.DSP_ERR_WORKSPACE
    assert lib.dsp_dhmm_score(*model, p, p, 0, 64, p, p, None, 0, None) == _hip.DSP_OK
    assert lib.dsp_dhmm_score(*model, p, p, 4, 64, None, None, None, 0, None) == _hip.DSP_OK
    assert lib.dsp_dhmm_align(*model, p, p, 4, 0, p, p, 4, p, p, p, big, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_dhmm_align(p, p, p, None, 3, 5, 64, p, p, 4, 64, p, p, 4, p, p, p, big, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_dhmm_align(*model, p, p, 4, 64, None, p, 4, p, p, p, big, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_dhmm_align(*model, p, p, 4, 64, p, p, 4, p, p, p, 8, None) == _hip.DSP_ERR_WORKSPACE
    assert lib.dsp_dhmm_align(*model, p, p, 4, 64, p, p, 0, p, p, None, 0, None) == _hip.DSP_OK
    assert lib.dsp_dhmm_align(*model, p, p, 4, 64, p, p, 4, None, None, None, 0, None) == _hip.DSP_OK
    acc = lambda cnt, ws, nws, C=3, K=64: lib.dsp_dhmm_accumulate(p, C, 5, K, p, p, 4, 64, p, p, 4, p, p, cnt, p, p, p, ws, nws,
                                                                  None)
    assert acc(None, p, big) == _hip.DSP_ERR_ARGS and acc(p, p, big, K=300) == _hip.DSP_ERR_ARGS
    assert acc(p, None, 0) == _hip.DSP_ERR_WORKSPACE and acc(p, p, 8) == _hip.DSP_ERR_WORKSPACE
    assert acc(p, None, 0, C=0) == _hip.DSP_OK
