"""Host tests of the vector-quantisation codebooks (csrc/vq.hip): the two forms of the
numpy restatement (tests/vq_reference.py) against each other and against exact integer arithmetic, the
numpy pieces of LBG training against hand-worked cases, and what the loaded library answers on the host
before any launch.  No test here needs a GPU."""
import ctypes

import numpy as np
import pytest

import vq_reference as V
from device_outputs import bits, csr


def same_bits(got, want):
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]


def random_corpus(seed, F, tied=False):
    """5 codebooks (K = 1, 2, 3, 7, 8 of Kmax = 8) and 23 sequences of 1 .. 9 frames; ``tied``: small
    integers, so that many frames have several codewords at the minimum."""
    rng = np.random.default_rng(seed)
    n_codes = np.array([1, 2, 3, 7, 8], np.int32)
    if tied:
        cb, x = rng.integers(-2, 3, (5, 8, F)).astype(np.float64), rng.integers(-2, 3, (23, 9, F)).astype(np.float64)
    else:
        cb, x = rng.normal(0, 1, (5, 8, F)), rng.normal(0, 1, (23, 9, F)) * rng.choice([1e-3, 1.0, 1e3], (23, 1, 1))
    n = rng.integers(1, 10, 23).astype(np.int32)
    n[:3] = [1, 9, 2]
    groups = [rng.integers(0, 23, k).tolist() for k in (9, 0, 14, 23, 5)]
    groups[0] += [3, 3]  # one sequence twice under one codebook
    return cb, n_codes, x, n, csr(groups)


@pytest.mark.parametrize("tied", (False, True))
@pytest.mark.parametrize("F", (1, 2, 3, 8))
def test_the_two_forms_agree(F, tied):
    cb, n_codes, x, n, (start, members) = random_corpus(10 + F, F, tied)
    s1, l1 = V.score_loop(cb, n_codes, x, n)
    s2, l2 = V.score(cb, n_codes, x, n)
    same_bits(s1, s2)
    assert np.array_equal(l1, l2) and np.isfinite(s1).all()
    d1, c1 = V.assign_loop(cb, n_codes, x, n, start, members)
    d2, c2 = V.assign(cb, n_codes, x, n, start, members)
    same_bits(d1, d2)
    assert np.array_equal(c1, c2)
    owner = np.repeat(np.arange(5), np.diff(start))
    same_bits(d1, s1[members, owner])
    assert ((c1 >= 0).sum(axis=1) == n[members]).all() and (c1.max(axis=1) < n_codes[owner]).all()
    a1 = V.accumulate_loop(cb, n_codes, x, n, start, members, c1, d1)
    a2 = V.accumulate(cb, n_codes, x, n, start, members, c2, d2)
    for g, w in zip(a1, a2):
        if g.dtype == np.float64:
            same_bits(g, w)
        else:
            assert np.array_equal(g, w)
    assert a1[2].tolist() == np.diff(start).tolist() and a1[1].sum() == n[members].sum()
    same_bits(a1[0][1], cb[1])  # the empty group: copied
    if tied:  # the tied corpus does have frames with two codewords at the minimum
        ties = 0
        for p in range(start[3], start[5]):
            q = cb[owner[p], :n_codes[owner[p]]]
            for t in range(n[members[p]]):
                d = ((x[members[p], t] - q) ** 2).sum(axis=1)
                ties += int((d == d.min()).sum() > 1)
        assert ties > 0


def test_invalid_members_and_codebooks():
    cb, n_codes, x, n, _ = random_corpus(20, 2)
    n, n_codes = n.copy(), n_codes.copy()
    n[[4, 5]] = [0, 10]
    n_codes[[1, 3]] = [0, 9]
    start, members = csr([[0, 4, 5, -1, 23, 1], [0, 1], [2, 4], [0], [5, 6]])
    for form in (V.assign_loop, V.assign):
        dist, code = form(cb, n_codes, x, n, start, members)
        assert np.isinf(dist[[1, 2, 3, 4, 6, 7, 9, 10, 11]]).all() and np.isfinite(dist[[0, 5, 8, 12]]).all()
        assert (code[np.isinf(dist)] == -1).all()
    for form in (V.score_loop, V.score):
        score, label = form(cb, n_codes, x, n)
        assert np.isinf(score[[4, 5]]).all() and np.isinf(score[:, [1, 3]]).all() and (label[[4, 5]] == -1).all()
        assert (label[[0, 1, 2, 3]] >= 0).all()


def test_codes_equal_exact_integer_arithmetic():
    """Integer frames and codewords: every fp64 sum is exact, so the code is the first minimum of the
    int64 brute force, and a tie goes to the smaller index."""
    rng = np.random.default_rng(30)
    K, F = 16, 2
    cb = rng.integers(-3, 4, (1, K, F))
    x = rng.integers(-3, 4, (40, 12, F))
    n = np.full(40, 12, np.int32)
    start, members = csr([list(range(40))])
    d = ((x[:, :, None, :] - cb[0][None, None]) ** 2).sum(axis=3)  # int64, exact
    want = np.argmin(d, axis=2)
    tied = (d == d.min(axis=2, keepdims=True)).sum(axis=2) > 1
    assert tied.mean() >= 0.25
    for form in (V.assign_loop, V.assign):
        dist, code = form(cb.astype(np.float64), [K], x.astype(np.float64), n, start, members)
        assert np.array_equal(code, want)
        assert np.array_equal(dist, d.min(axis=2).sum(axis=1).astype(np.float64))
    # an explicit tie: two identical codewords, the smaller index wins
    two = np.array([[[1.0, 2.0], [1.0, 2.0], [0.0, 0.0]]])
    assert V.frame_loop(two[0], np.array([1.0, 1.0]))[1] == 0 and V.nearest(two[0], np.array([[1.0, 1.0]]))[1][0] == 0


def test_accumulate_keeps_a_negative_zero():
    """A cell fed only -0.0 frames, other members contributing none to it: -0.0 (adding a member's 0.0
    for an empty cell would turn it into +0.0)."""
    x = np.zeros((3, 2, 1))
    x[0, :, 0] = [1.0, 2.0]
    x[1, :, 0] = [-0.0, -0.0]
    x[2, :, 0] = [3.0, 4.0]
    n = np.array([2, 2, 2], np.int32)
    start, members = csr([[0, 1, 2]])
    code = np.array([[0, 0], [1, 1], [0, 0]], np.int32)
    prev = np.full((1, 3, 1), 7.0)
    for form in (V.accumulate_loop, V.accumulate):
        cen, cnt, nv, total = form(prev, [3], x, n, start, members, code, np.array([1.0, 2.0, 3.0]))
        assert cen[0, 0, 0] == 2.5 and cen[0, 1, 0] == 0.0 and np.signbit(cen[0, 1, 0]) and cen[0, 2, 0] == 7.0
        assert cnt.tolist() == [[4, 2, 0]] and nv.tolist() == [1 + 2] and total.tolist() == [6.0]


def test_accumulate_skips_a_member_with_a_bad_code():
    cb, n_codes, x, n, (start, members) = random_corpus(40, 2)
    dist, code = V.assign(cb, n_codes, x, n, start, members)
    bad = code.copy()
    p = int(start[3]) + 2
    bad[p, n[members[p]] - 1] = n_codes[3]  # one code out of range: the member is skipped whole
    a1 = V.accumulate_loop(cb, n_codes, x, n, start, members, bad, dist)
    a2 = V.accumulate(cb, n_codes, x, n, start, members, bad, dist)
    keep = np.delete(np.arange(len(members)), p)
    start2 = start.copy()
    start2[4:] -= 1
    a3 = V.accumulate(cb, n_codes, x, n, start2, members[keep], code[keep], dist[keep])
    assert a1[2][3] == start[4] - start[3] - 1
    for g, w, v in zip(a1, a2, a3):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)) and np.array_equal(g.view(np.uint8), v.view(np.uint8))


def test_split_and_repair_hand_worked():
    from src.pipeline import vq_repair_empty, vq_split
    cb = np.array([[[1.0, -2.0], [0.5, 0.25]]])
    want = np.array([[[1.5, -1.5], [0.5, -2.5], [1.0, 0.75], [0.0, -0.25]]])
    for f in (vq_split, V.split):
        same_bits(f(cb, 0.5), want)
        same_bits(f(cb[0], 0.5), want[0])
    inexact = np.array([[[0.1, 1e17]]])
    same_bits(vq_split(inexact, 0.01), np.array([[[0.1 + 0.01, 1e17], [0.1 - 0.01, 1e17]]]))
    books = np.arange(8.0).reshape(1, 4, 2)
    for f in (vq_repair_empty, V.repair_empty):
        # no donor: no cell holds two frames, the empty cells stay as they are
        cb2, cnt2 = f(books, [[1, 0, 1, 0]], [4], 0.5)
        same_bits(cb2, books)
        assert cnt2.tolist() == [[1, 0, 1, 0]]
        # donor tie: cells 0 and 2 both hold 6, the smaller index gives
        cb2, cnt2 = f(books, [[6, 0, 6, 3]], [4], 0.5)
        same_bits(cb2, np.array([[[-0.5, 0.5], [0.5, 1.5], [4.0, 5.0], [6.0, 7.0]]]))
        assert cnt2.tolist() == [[3, 3, 6, 3]]
        # two empty cells drawing from one donor: 9 -> 5 + 4, then the 5 -> 3 + 2 (cell 3 holds only 4)
        cb2, cnt2 = f(books, [[9, 0, 0, 4]], [4], 0.5)
        same_bits(cb2, np.array([[[-1.0, 0.0], [0.5, 1.5], [0.0, 1.0], [6.0, 7.0]]]))
        assert cnt2.tolist() == [[3, 4, 2, 4]]
        # cells behind n_codes are neither repaired nor donors
        cb2, cnt2 = f(books, [[0, 1, 0, 50]], [3], 0.5)
        same_bits(cb2, books)
        assert cnt2.tolist() == [[0, 1, 0, 50]]
        # the inputs are not written
        assert books[0, 0, 0] == 0.0


def test_reference_fit_trains_and_repairs():
    """The restatement's whole fit on a tiny corpus: the totals do not rise within a level where no repair
    fired, and a class of many equal frames makes vq_repair_empty fire."""
    rng = np.random.default_rng(50)
    X = rng.normal(0, 1, (12, 6, 2))
    X[1::2] += 4.0
    X[0::2] = np.round(X[0::2] / 3.0) * 3.0  # class 0: fewer distinct frames than codewords, cells run empty
    n = rng.integers(3, 7, 12).astype(np.int32)
    codes = np.arange(12) % 2
    cb, cnt, totals, repairs = V.fit(X, n, codes, 8, n_iter=4, eps=0.01)
    assert cb.shape == (2, 8, 2) and cnt.shape == (2, 8) and totals.shape[1] == 2 and 6 <= len(totals) <= 12
    assert cnt.sum(axis=1).tolist() == [n[codes == c].sum() for c in range(2)]
    assert repairs > 0 and np.isfinite(cb).all()
    one = V.fit(X, n, codes, 1)
    assert one[2].shape == (0, 2) and np.allclose(one[0][1, 0], X[1::2][np.arange(6)[None, :] < n[1::2][:, None]].mean(axis=0))


def test_create_classifier_validates_without_a_device():
    from src.models import SequenceClassifier, VqClassifier, create_classifier
    from src.pipeline import VQ_MAX_CODES
    clf = create_classifier('vq')
    assert isinstance(clf, VqClassifier) and isinstance(clf, SequenceClassifier) and VQ_MAX_CODES == 256
    assert (clf.n_codes, clf.n_iter, clf.eps, clf.normalize) == (16, 10, 0.01, True)
    assert create_classifier('vq', n_codes=1).n_codes == 1 and create_classifier('vq', n_codes=256).n_codes == 256
    for bad in (dict(n_codes=3), dict(n_codes=512), dict(n_codes=0), dict(n_codes=2.0), dict(n_iter=0), dict(eps=0.0),
                dict(eps=float("inf"))):
        with pytest.raises(ValueError):
            create_classifier('vq', **bad)
    for name in ("fit", "predict", "score_samples", "evaluate"):
        assert callable(getattr(clf, name))
    with pytest.raises(NotImplementedError):
        clf.kneighbors([np.zeros((3, 2))])


def test_fit_needs_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from src import _hip
    from src.models import create_classifier
    from src.pipeline import vq_assign, vq_score
    seqs = [np.random.default_rng(i).normal(0, 1, (5, 2)) for i in range(6)]
    with pytest.raises(_hip.HipError):
        create_classifier('vq', n_codes=2).fit(seqs, [0, 1] * 3)
    with pytest.raises(_hip.HipError):
        vq_score(np.zeros((1, 1, 2)), [1], np.zeros((1, 5, 2)), [5])
    with pytest.raises(_hip.HipError):
        vq_assign(np.zeros((1, 1, 2)), [1], np.zeros((1, 5, 2)), [5], assign=[0])


def test_abi_argument_checks():
    """The plan's bounds and the NULL checks, answered on the host before any launch."""
    from src import _hip
    lib = _hip.load_library()
    wb = lib.dsp_vq_workspace_bytes
    assert wb(10, 100, 100, 64, 2, 16) > 0 and wb(10, 100, 0, 1024, 8, 256) > 0 and wb(0, 0, 0, 1, 1, 1) > 0
    for args in ((10, 100, 100, 64, 9, 16), (10, 100, 100, 1025, 2, 16), (10, 100, 100, 64, 2, 0), (10, 100, 100, 64, 2, 257),
                 (10, 100, 100, 64, 0, 16), (10, 100, 100, 0, 2, 16), (-1, 100, 100, 64, 2, 16), ((1 << 20) + 1, 1, 1, 64, 2, 16)):
        assert wb(*args) == 0, args
    # one pair chunk holds 128 MiB of sums, counts and validity: the workspace stops growing with P there
    chunk = (128 << 20) // (256 * (4 + 8 * 8) + 4)
    assert chunk == 7708 and wb(2, 50, chunk - 1, 3, 8, 256) < wb(2, 50, chunk, 3, 8, 256) == wb(2, 50, 8000, 3, 8, 256)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 8)
    big = 1 << 30
    score = lambda cb=p, x=p, N=4, F=2, Kmax=16, out=p, ws=p, nws=big: lib.dsp_vq_score(cb, p, 3, Kmax, x, p, N, 64, F, out, p, ws, nws, None)
    assert score(F=9) == _hip.DSP_ERR_ARGS and score(Kmax=257) == _hip.DSP_ERR_ARGS and score(Kmax=0) == _hip.DSP_ERR_ARGS
    assert score(cb=None) == _hip.DSP_ERR_ARGS and score(x=None) == _hip.DSP_ERR_ARGS
    assert score(ws=None, nws=0) == _hip.DSP_ERR_WORKSPACE and score(nws=8) == _hip.DSP_ERR_WORKSPACE
    assert score(N=0, ws=None, nws=0) == _hip.DSP_OK
    assert lib.dsp_vq_score(p, p, 3, 16, p, p, 4, 64, 2, None, None, None, 0, None) == _hip.DSP_OK
    assign = lambda cb=p, gs=p, mem=p, P=4, T=64, ws=p, nws=big: lib.dsp_vq_assign(cb, p, 3, 16, p, p, 4, T, 2, gs, mem, P, p, p, ws, nws, None)
    assert assign(T=1025) == _hip.DSP_ERR_ARGS and assign(cb=None) == _hip.DSP_ERR_ARGS
    assert assign(gs=None) == _hip.DSP_ERR_ARGS and assign(mem=None) == _hip.DSP_ERR_ARGS
    assert assign(nws=8) == _hip.DSP_ERR_WORKSPACE and assign(ws=None, nws=0) == _hip.DSP_ERR_WORKSPACE
    assert assign(P=0, ws=None, nws=0) == _hip.DSP_OK
    acc = lambda prev=p, cen=q, code=p, C=3, ws=p, nws=big: lib.dsp_vq_accumulate(prev, p, C, 16, p, p, 4, 64, 2, p, p, 4, code, p, cen, p, p, p,
                                                                                  ws, nws, None)
    assert acc(prev=None) == _hip.DSP_ERR_ARGS and acc(cen=None) == _hip.DSP_ERR_ARGS and acc(code=None) == _hip.DSP_ERR_ARGS
    assert acc(cen=p) == _hip.DSP_ERR_ARGS  # centroid == cb_prev
    assert acc(ws=None, nws=0) == _hip.DSP_ERR_WORKSPACE and acc(nws=8) == _hip.DSP_ERR_WORKSPACE
    assert acc(C=0, ws=None, nws=0) == _hip.DSP_OK
