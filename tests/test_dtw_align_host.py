"""CPU checks of the DTW alignment / DBA feature: the numpy restatements of the path
(tests/dtw_align_reference.py) against each other and against what a path must satisfy, the new
exports and their host argument checks, and the host side of TemplateClassifier."""
import ctypes
import inspect

import numpy as np
import pytest

import dtw_align_reference as A
import dtw_reference as R


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


tie_case = A.tie_case


def table_pairs(F):
    """A spread of the case table's pairs: every forced length on a's side, several on b's."""
    a, la, b, lb = R.table_case(F)
    return [(a[q, :la[q]], b[r, :lb[r]]) for q in range(len(a)) for r in range(q % 5, len(b), 5)]


def check_path(x, y, window, d2, path):
    """The range invariants, the band and the cost along the path (A.check_path) on the path's
    ranges, which are the whole path."""
    lo, hi = A.ranges(path, len(x) + 3)
    assert np.array_equal(A.check_path(x, y, window, d2, lo, hi), path)


@pytest.mark.parametrize("window", R.TABLE_WINDOWS)
@pytest.mark.parametrize("F", R.TABLE_F)
def test_backtrace_forms_agree_on_the_table_case(F, window):
    for x, y in table_pairs(F):
        d_s, p_s = A.align_pair(x, y, window, "scalar")
        d_w, p_w = A.align_pair(x, y, window, "wavefront")
        assert bits(d_s) == bits(d_w) and np.array_equal(p_s, p_w)
        assert bits(np.sqrt(d_s)) == bits(R.dtw_scalar(x, y, window))
        check_path(x, y, window, d_s, p_s)


@pytest.mark.parametrize("window", (-1, 2))
@pytest.mark.parametrize("F", (1, 2))
def test_backtrace_forms_agree_on_ties(F, window):
    seqs = tie_case(F, 60 + F)
    differ = 0
    for x in seqs:
        for y in seqs:
            d_s, p_s = A.align_pair(x, y, window, "scalar")
            d_w, p_w = A.align_pair(x, y, window, "wavefront")
            assert bits(d_s) == bits(d_w) and np.array_equal(p_s, p_w)
            check_path(x, y, window, d_s, p_s)
            d_t, p_t = A.align_pair(y, x, window, "scalar")
            assert bits(d_t) == bits(d_s)  # the distance is symmetric, the tie rule is not
            differ += not np.array_equal(p_t[:, ::-1], p_s)
    assert differ > 0


def test_hand_worked_cases():
    _, p = A.align_pair([[0.0], [0.0]], [[0.0]])
    lo, hi = A.ranges(p, 2)
    assert lo.tolist() == [0, 0] and hi.tolist() == [0, 0]
    # the swap: one a frame matched to both b frames
    _, p = A.align_pair([[0.0]], [[0.0], [0.0]])
    lo, hi = A.ranges(p, 1)
    assert lo.tolist() == [0] and hi.tolist() == [1]
    # all zeros, 2 x 2: every predecessor ties, the diagonal is first
    _, p = A.align_pair(np.zeros((2, 1)), np.zeros((2, 1)))
    assert p.tolist() == [[0, 0], [1, 1]]
    # 3 x 2 of zeros: from (2, 1) the diagonal, then from (1, 0) the a-step (the diagonal is outside the grid)
    _, p = A.align_pair(np.zeros((3, 1)), np.zeros((2, 1)))
    assert p.tolist() == [[0, 0], [1, 0], [2, 1]]
    _, p = A.align_pair(np.zeros((2, 1)), np.zeros((3, 1)))
    assert p.tolist() == [[0, 0], [0, 1], [1, 2]]
    # a = (0, 1, 0), b = (1, 0, 1): D(1,2) = D(2,1) = 1 < D(1,1) = 2 at the end cell, the a-step comes
    # before the b-step; the swap takes the other branch: the rule is stated in a / b indices
    x, y = np.array([[0.0], [1.0], [0.0]]), np.array([[1.0], [0.0], [1.0]])
    _, p = A.align_pair(x, y)
    _, q = A.align_pair(y, x)
    assert p.tolist() == [[0, 0], [0, 1], [1, 2], [2, 2]] and q.tolist() == [[0, 0], [0, 1], [1, 2], [2, 2]]
    assert q[:, ::-1].tolist() != p.tolist()


def test_dba_restatement_and_medoid_rule():
    """One update by hand, the copy rules, the fixed point, and the medoid's tie to the earliest."""
    seqs, n = R.pad([np.array([[0.0], [2.0], [4.0]]), np.array([[2.0], [4.0]]), np.array([[9.0]])], T=4)
    tmpl, lt = R.pad([np.array([[1.0], [3.0]]), np.array([[5.0]]), np.array([[7.0]])], T=3)
    n2 = n.copy()
    n2[2] = 9  # an invalid member: skipped
    out, inertia = A.dba_update(tmpl, lt, seqs, n2, [0, 3, 3, 4], [0, 1, 2, 2])
    # template 0 = (1, 3): s0 = (0, 2, 4) aligns 0, 2 | 4 (D(1,2) ties between the diagonal and the
    # b-step: the diagonal), s1 = (2, 4) aligns 2 | 4
    assert out[0].tolist() == [[((0.0 + 2.0) + 2.0) / 3], [(4.0 + 4.0) / 2], [0.0]]
    assert inertia[0] == (1.0 + 1.0 + 1.0) + (1.0 + 1.0)
    assert np.array_equal(bits(out[1:]), bits(tmpl[1:])) and inertia[1:].tolist() == [0.0, 0.0]
    same = np.repeat(seqs[:1], 5, axis=0)
    out, inertia = A.dba_update(same[:1], n[:1], same, np.repeat(n[:1], 5), [0, 5], np.arange(5))
    assert np.array_equal(bits(out), bits(same[:1])) and inertia.tolist() == [0.0]
    X, nx = R.pad([np.array([[0.0]]), np.array([[1.0]]), np.array([[1.0]]), np.array([[2.0]])])
    assert A.medoid(X, nx, np.arange(4)) == 1 and A.medoid(X, nx, np.arange(4), candidates=1) == 0
    assert A.medoid(X, nx, np.array([3, 2, 0])) == 2
    from src.models import medoid_index
    d = R.dtw_pairwise(X, nx, X, nx)
    assert medoid_index(d * d) == 1


def test_exports_are_typed_and_check_their_arguments():
    from src import _hip
    lib = _hip.load_library()
    assert lib.dsp_abi_version() == 6 and _hip.ABI_VERSION == 6
    for name in ("dsp_dtw_align_workspace_bytes", "dsp_dtw_align", "dsp_dtw_dba_update"):
        assert name in _hip.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.dsp_dtw_align_workspace_bytes.restype is ctypes.c_size_t
    assert lib.dsp_dtw_align.argtypes[12] is ctypes.c_int64 and lib.dsp_dtw_dba_update.argtypes[12] is ctypes.c_int64  # P
    w = lib.dsp_dtw_align_workspace_bytes  # (Na, P, Ta, Tb, F)
    assert w(19, 37, 70, 70, 3) > 0 and w(10, 8000, 1024, 1024, 8) > 0 and w(1, 1, 1, 1, 1) > 0
    # a wave's words and edge hold one tile: ceil(Ta / 32) + 1 columns of Tb x 64 x 8 bytes
    assert w(1, 64, 70, 70, 3) >= (3 + 1) * 70 * 64 * 8
    # bounded whatever P and Na are: <= 1 GiB of words and edges, 1024 padded sequences (66 MiB),
    # ranges and sums of one pair chunk (128 MiB + its distances) and one chunk's counts (32 MiB)
    big = w(10 ** 9, (1 << 31) - 1, 1024, 1024, 8)
    assert 0 < big <= (1024 + 66 + 128 + 1 + 32 + 1) << 20
    assert w(10, (1 << 31) - 1, 33, 33, 2) == w(10, 1 << 30, 33, 33, 2) <= (1024 + 128 + 8) << 20
    for bad in ((19, 37, 70, 70, 0), (19, 37, 70, 70, 9), (19, 37, 0, 70, 3), (19, 37, 70, 0, 3), (19, 37, 1025, 70, 3),
                (19, 37, 70, 1025, 3), (-1, 37, 70, 70, 3), (19, -1, 70, 70, 3), (19, 1 << 31, 70, 70, 3)):
        assert w(*bad) == 0, bad
    # host argument checks come before any launch
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    E, W, OK = _hip.DSP_ERR_ARGS, _hip.DSP_ERR_WORKSPACE, _hip.DSP_OK
    al = lambda Ta=70, Tb=70, F=3, ws=p, nws=1 << 40, a=p, lo=p, hi=p, P=37, Nb=37, dist=p, Na=19: lib.dsp_dtw_align(
        a, p, Na, Ta, p, p, Nb, Tb, F, -1, p, p, P, dist, lo, hi, ws, nws, None)
    assert al(F=0) == E and al(F=9) == E and al(Ta=0) == E and al(Tb=0) == E and al(Ta=1025) == E and al(Tb=1025) == E
    assert al(a=None) == E and al(P=-1) == E and al(P=1 << 31) == E and al(Nb=-1) == E and al(Na=-1) == E
    assert al(lo=None) == E and al(hi=None) == E  # both or neither
    assert al(nws=w(19, 37, 70, 70, 3) - 1) == W and al(ws=None) == W
    assert al(P=0, ws=None, nws=0) == OK and al(Na=0, ws=None, nws=0) == OK  # nothing to do
    assert al(dist=None, lo=None, hi=None, ws=None, nws=0) == OK  # nothing asked for
    buf2 = ctypes.create_string_buffer(64)
    p2 = ctypes.cast(buf2, ctypes.c_void_p)
    db = lambda Tt=70, Ts=70, F=3, ws=p, nws=1 << 40, t=p, out=p2, P=37, C=3: lib.dsp_dtw_dba_update(
        t, p, C, Tt, p, p, 37, Ts, F, -1, p, p, P, out, p, ws, nws, None)
    assert db(F=0) == E and db(F=9) == E and db(Tt=0) == E and db(Ts=1025) == E and db(P=-1) == E
    assert db(t=None) == E and db(out=None) == E and db(out=p) == E  # the output is not the input
    assert db(nws=w(3, 37, 70, 70, 3) - 1) == W and db(ws=None) == W
    assert db(C=0, ws=None, nws=0) == OK


def _seqs(seed, N=12, F=2):
    rng = np.random.default_rng(seed)
    seqs = [rng.normal(0, 1, (int(n), F)) * [100.0, 0.01][:F] + [5.0, -1.0][:F] for n in rng.integers(2, 9, N)]
    return seqs, np.arange(N) % 3 * 5 + 2


def test_template_classifier_host_side(monkeypatch):
    """Constructing and input validation need no device; fit is an accelerated entry point with no
    host fall-back."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from src import _hip
    from src.models import SequenceClassifier, TemplateClassifier, create_classifier
    clf = create_classifier("dtw_template")
    assert isinstance(clf, TemplateClassifier) and isinstance(clf, SequenceClassifier)
    assert (clf.n_iter, clf.window, clf.normalize, clf.medoid_candidates, clf.n_neighbors) == (10, None, True, 256, 1)
    sig = inspect.signature(TemplateClassifier.__init__)
    assert list(sig.parameters)[1:] == ["n_iter", "window", "normalize", "medoid_candidates"]
    clf = create_classifier("dtw_template", n_iter=3, window=4, normalize=False, medoid_candidates=5)
    assert (clf.n_iter, clf.window, clf.normalize, clf.medoid_candidates) == (3, 4, False, 5)
    with pytest.raises(ValueError):
        TemplateClassifier(n_iter=-1)
    with pytest.raises(ValueError):
        TemplateClassifier(medoid_candidates=0)
    seqs, y = _seqs(4)
    padded, n = R.pad(seqs)
    with pytest.raises(ValueError, match="lengths"):
        TemplateClassifier().fit(padded, y)
    with pytest.raises(ValueError):
        TemplateClassifier().fit(seqs, y[:-1])
    bad = [s.copy() for s in seqs]
    bad[3][1, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        TemplateClassifier().fit(bad, y)
    with pytest.raises(_hip.HipError):
        TemplateClassifier().fit(seqs, y)
    with pytest.raises(_hip.HipError):
        TemplateClassifier().fit(padded, y, lengths=n)


def test_pair_list_from_assign_and_compare_defaults():
    from src.pipeline import _dtw_groups
    start, members = _dtw_groups(None, [2, -1, 0, 2, 0, 2], 4, 6)
    assert start.tolist() == [0, 2, 2, 5, 5] and members.tolist() == [2, 4, 0, 3, 5]
    assert start.dtype == np.int32 and members.dtype == np.int32
    start, members = _dtw_groups(([0, 1, 3], [5, 5, 0]), None, 2, 6)
    assert start.tolist() == [0, 1, 3] and members.tolist() == [5, 5, 0]
    for groups, assign in ((None, None), (([0, 1], [0]), [0]), (([0, 2], [0]), None), (([1, 1], [0]), None),
                           (None, [0, 4, 0, 0, 0, 0]), (None, [0, 0])):
        with pytest.raises(ValueError):
            _dtw_groups(groups, assign, 4 if groups is None else 1, 6)
    import compare_feature_methods as cfm
    sig = inspect.signature(cfm.compare)
    assert sig.parameters["dtw"].default is False and sig.parameters["dtw_template"].default is False
    assert list(sig.parameters)[:5] == ["data_dir", "classifiers", "test_size", "random_state", "dtw"]
