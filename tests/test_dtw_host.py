"""CPU checks of the DTW classifier: the numpy restatements of the definition
(tests/dtw_reference.py) against each other bit for bit and against closed forms, the new exports
and their host argument checks, and the host side of SequenceClassifier."""
import ctypes
import inspect

import numpy as np
import pytest

import dtw_reference as R


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("window", R.TABLE_WINDOWS)
@pytest.mark.parametrize("F", R.TABLE_F)
def test_restatements_agree_bit_for_bit(F, window):
    """The scalar triple loop, the form vectorised over the pairs and the wavefront form on the case
    table that tests/test_gpu_dtw.py runs on the device (19 x 37 pairs, T = 70, every forced length)."""
    a, la, b, lb = R.table_case(F)
    vec = R.dtw_pairwise(a, la, b, lb, window)
    one = np.array([[R.dtw_scalar(a[q, :la[q]], b[r, :lb[r]], window) for r in range(len(b))] for q in range(len(a))])
    wav = np.array([[R.dtw_wavefront(a[q, :la[q]], b[r, :lb[r]], window) for r in range(len(b))]
                    for q in range(len(a))])
    assert np.isfinite(vec).all()
    assert np.array_equal(bits(vec), bits(one)) and np.array_equal(bits(vec), bits(wav))


def test_invalid_lengths_in_the_restatement():
    a, la, b, lb = R.case(4, 5, 6, 2, seed=1)
    la[1], lb[0], lb[3] = 0, 7, -1
    d = R.dtw_pairwise(a, la, b, lb)
    assert np.isinf(d[1]).all() and np.isinf(d[:, 0]).all() and np.isinf(d[:, 3]).all()
    assert np.isfinite(d[[0, 2, 3]][:, [1, 2, 4]]).all()


def test_closed_forms():
    rng = np.random.default_rng(3)
    a, b = rng.normal(0, 1, (23, 3)), rng.normal(0, 1, (37, 3))
    for f in (R.dtw_scalar, R.dtw_wavefront):
        assert f(a, a) == 0.0
        assert f(a, np.repeat(a, 3, axis=0)) == 0.0
        # n == 1: the sequentially added costs
        acc = 0.0
        for j in range(len(b)):
            c = 0.0
            for k in range(3):
                t = a[0, k] - b[j, k]
                c = c + t * t
            acc = c if j == 0 else c + acc
        assert bits(f(a[:1], b)) == bits(np.sqrt(acc))
        # symmetric in its arguments, band or not
        for w in (-1, 0, 5):
            assert bits(f(a, b, w)) == bits(f(b, a, w))
        # n == m, window 0: the diagonal
        b2 = b[:23]
        acc = None
        for i in range(23):
            c = 0.0
            for k in range(3):
                t = a[i, k] - b2[i, k]
                c = c + t * t
            acc = c if acc is None else c + acc
        assert bits(f(a, b2, 0)) == bits(np.sqrt(acc))
        # a window below |n - m| behaves as |n - m|
        for w in (0, 3, 13):
            assert bits(f(a, b, w)) == bits(f(a, b, 14))
        assert f(a, b, 14) >= f(a, b, 20) >= f(a, b, -1)
    pa, la = R.pad([a, a[:1]])
    pb, lb = R.pad([b, a, b2])
    d = R.dtw_pairwise(pa, la, pb, lb)
    assert d[0, 1] == 0.0 and bits(d[0, 0]) == bits(R.dtw_scalar(a, b)) and bits(d[1, 0]) == bits(R.dtw_scalar(a[:1], b))


def test_knn_restatement_rules():
    d = np.array([[2.0, 1.0, 1.0, np.inf, 0.5], [np.inf, np.inf, 3.0, np.inf, np.inf]])
    labels = np.array([4, 2, 1, 0, 3])
    idx, dist, pred = R.knn_from_dist(d, 3, labels)
    assert idx.tolist() == [[4, 1, 2], [2, -1, -1]] and dist[1].tolist() == [3.0, np.inf, np.inf]
    assert pred.tolist() == [1, 1]  # a three-way tie: the smallest label
    idx, _, _ = R.knn_from_dist(d[:1], 2, labels, self_offset=4)
    assert idx.tolist() == [[1, 2]]


def test_exports_are_typed_and_check_their_arguments():
    from src import _hip
    lib = _hip.load_library()
    assert lib.dsp_abi_version() == 6 and _hip.ABI_VERSION == 6
    for name in ("dsp_dtw_workspace_bytes", "dsp_dtw_pairwise", "dsp_dtw_knn"):
        assert name in _hip.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.dsp_dtw_workspace_bytes.restype is ctypes.c_size_t
    assert lib.dsp_dtw_knn.argtypes[12] is ctypes.c_int64  # self_offset
    w = lib.dsp_dtw_workspace_bytes  # (Nr, Nq, Tr, Tq, F, k)
    assert w(37, 19, 70, 70, 3, 3) >= 19 * 37 * 8 and w(8000, 2000, 1024, 1024, 8, 32) > 0 and w(5, 5, 1, 1, 1, 1) > 0
    # bounded: edge columns <= 256 MiB, padded queries and distance rows of one chunk of <= 1024 queries
    assert w(8000, 10 ** 9, 1024, 1024, 8, 32) == w(8000, 1024, 1024, 1024, 8, 32) <= (256 + 72 + 64) << 20
    for bad in ((37, 19, 70, 70, 0, 3), (37, 19, 70, 70, 9, 3), (37, 19, 0, 70, 3, 3), (37, 19, 70, 0, 3, 3),
                (37, 19, 1025, 70, 3, 3), (37, 19, 70, 1025, 3, 3), (37, 19, 70, 70, 3, 0), (37, 19, 70, 70, 3, 33),
                (1 << 31, 19, 70, 70, 3, 3), (37, -1, 70, 70, 3, 3)):
        assert w(*bad) == 0, bad
    # host argument checks come before any launch
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    E, W = _hip.DSP_ERR_ARGS, _hip.DSP_ERR_WORKSPACE
    pw = lambda Tq=70, Tr=70, F=3, ws=p, nws=1 << 30, a=p: lib.dsp_dtw_pairwise(
        a, p, 19, Tq, p, p, 37, Tr, F, -1, p, ws, nws, None)
    assert pw(F=0) == E and pw(F=9) == E and pw(Tq=0) == E and pw(Tr=0) == E and pw(Tq=1025) == E and pw(Tr=1025) == E
    assert pw(a=None) == E
    assert pw(nws=8) == W and pw(ws=None) == W
    assert lib.dsp_dtw_pairwise(p, p, 0, 70, p, p, 37, 70, 3, -1, p, None, 0, None) == _hip.DSP_OK  # nothing to do
    kn = lambda Tq=70, Tr=70, F=3, k=3, ws=p, nws=1 << 30, idx=p: lib.dsp_dtw_knn(
        p, p, p, 37, Tr, p, p, 19, Tq, F, -1, k, -1, 4, idx, p, None, ws, nws, None)
    assert kn(F=0) == E and kn(F=9) == E and kn(Tq=0) == E and kn(Tr=1025) == E and kn(k=0) == E and kn(k=33) == E
    assert kn(idx=None) == E
    assert kn(nws=w(37, 19, 70, 70, 3, 3) - 1) == W and kn(ws=None) == W
    assert lib.dsp_dtw_knn(p, p, p, 37, 70, p, p, 0, 70, 3, -1, 3, -1, 4, None, None, None, None, 0, None) == _hip.DSP_OK


def _seqs(seed, N=12, F=2):
    rng = np.random.default_rng(seed)
    seqs = [rng.normal(0, 1, (int(n), F)) * [100.0, 0.01][:F] + [5.0, -1.0][:F] for n in rng.integers(2, 9, N)]
    return seqs, np.arange(N) % 3 * 5 + 2


def test_sequence_classifier_host_side(monkeypatch):
    """fit needs no device; list and padded + lengths input and the pooled normalisation equal a
    direct numpy computation; predict is an accelerated entry point with no host fall-back."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from src import _hip
    from src.models import SequenceClassifier, create_classifier
    seqs, y = _seqs(4)
    clf = create_classifier("dtw_knn", n_neighbors=3).fit(seqs, y)
    assert isinstance(clf, SequenceClassifier) and clf.n_neighbors == 3 and clf.window is None and clf.normalize
    frames = np.concatenate(seqs)
    mean, std = np.mean(frames, axis=0), np.std(frames, axis=0)
    assert np.array_equal(clf.mean_, mean) and np.array_equal(clf.std_, std)
    assert clf.classes_.tolist() == [2, 7, 12] and clf._codes.tolist() == (np.arange(12) % 3).tolist()
    for i, s in enumerate(seqs):
        assert clf._fit_n[i] == len(s)
        assert np.array_equal(clf._fit_X[i, :len(s)], (s - mean) / std) and not clf._fit_X[i, len(s):].any()
    padded, n = R.pad(seqs, T=11)
    padded[np.arange(11)[None, :] >= n[:, None]] = 7.5  # padding is not a frame, whatever it holds
    clf2 = SequenceClassifier().fit(padded, y, lengths=n)
    assert np.array_equal(clf2.mean_, mean) and np.array_equal(clf2.std_, std)
    assert np.array_equal(clf2._fit_X[:, :clf._fit_X.shape[1]], clf._fit_X) and not clf2._fit_X[:, clf._fit_X.shape[1]:].any()
    const = [np.ones((4, 2)) * [3.0, 1.0]] * 3
    c3 = SequenceClassifier(n_neighbors=1).fit(const, [0, 1, 2])
    assert c3.std_.tolist() == [1.0, 1.0] and not c3._fit_X.any()  # std == 0 -> 1
    raw = SequenceClassifier(normalize=False).fit(seqs, y)
    assert np.array_equal(raw._fit_X[0, :len(seqs[0])], seqs[0]) and not hasattr(raw, "mean_")
    for call in (clf.predict, clf.kneighbors, lambda X: clf.evaluate(X, y)):
        with pytest.raises(_hip.HipError):
            call(seqs)


def test_sequence_classifier_rejects_bad_input():
    from src.models import SequenceClassifier
    seqs, y = _seqs(5)
    padded, n = R.pad(seqs)
    with pytest.raises(ValueError, match="lengths"):
        SequenceClassifier().fit(padded, y)
    with pytest.raises(ValueError, match="n_neighbors"):
        SequenceClassifier(n_neighbors=13).fit(seqs, y)
    bad = [s.copy() for s in seqs]
    bad[3][1, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        SequenceClassifier().fit(bad, y)
    bad[3][1, 0] = np.inf
    with pytest.raises(ValueError, match="NaN"):
        SequenceClassifier().fit(bad, y)
    clf = SequenceClassifier().fit(seqs, y)
    with pytest.raises(ValueError, match="NaN"):
        clf.predict(bad)
    with pytest.raises(ValueError, match="lengths"):
        clf.predict(padded)
    with pytest.raises(ValueError):
        SequenceClassifier().fit(padded, y, lengths=n + 100)
    with pytest.raises(ValueError):
        SequenceClassifier().fit(seqs, y[:-1])
    nanpad = padded.copy()
    nanpad[np.arange(padded.shape[1])[None, :] >= n[:, None]] = np.nan  # NaN in the padding only: not a frame
    SequenceClassifier().fit(nanpad, y, lengths=n)


def test_compare_keeps_its_default():
    import compare_feature_methods as cfm
    sig = inspect.signature(cfm.compare)
    assert sig.parameters["dtw"].default is False
    assert list(sig.parameters)[:4] == ["data_dir", "classifiers", "test_size", "random_state"]
    assert set(cfm.CLASSIFIERS) == {"KNN", "SVM", "Decision Tree"}
