"""What the GPU tests of the three scikit-learn-backed classifiers share (tests/test_gpu_svc.py,
tests/test_gpu_nb_tree.py): a query cut into two launches, and a classifier given device rows (a plain
helper module like tests/crop_frame_cases.py: no test, no fixture)."""
import numpy as np
import torch


def check_two_launches(monkeypatch, Index, entry, nq_arg, model, X, tie_X, **values):
    """1025 rows -- a near tie, 1023 ordinary rows, a near tie -- through an index whose WORKSPACE_CAP
    of 1 leaves 1024 rows per launch: a launch of 1024 rows and a launch of exactly one, an uncertifiable
    row in each.  The counts add up, and pred, certified and the bits of the values (``with_dec=True`` /
    ``with_jll=True``) are those of an index with the default cap, which takes one launch.
    ``entry`` is the C call of a launch and ``nq_arg`` the position of its row count."""
    from src import _hip
    rows = np.concatenate([tie_X[:1], np.tile(X, (-(-1023 // len(X)), 1))[:1023], tie_X[1:2]])
    assert rows.shape[0] == 1025
    launched, call = [], getattr(_hip.lib(), entry)
    monkeypatch.setattr(_hip.lib(), entry, lambda *a: launched.append(a[nq_arg]) or call(*a))
    cut, stats = Index(model), {}
    cut.WORKSPACE_CAP = 1
    got = [t.cpu().numpy() for t in cut.query(rows, stats=stats, **values)]
    assert launched == [1024, 1] and stats == {"uncertified": 2}
    assert np.flatnonzero(got[2] == 0).tolist() == [0, 1024]
    want = [t.cpu().numpy() for t in Index(model).query(rows, stats=stats, **values)]
    assert launched == [1024, 1, 1025] and stats == {"uncertified": 2}
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert got[1].shape == want[1].shape and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))


def check_device_rows(clf, X, uncertified):
    """predict (and apply, for a tree) of float64 device rows: the model's own answer for the host rows,
    and the same count of rows left to the model as with host rows."""
    methods = ["predict"] + (["apply"] if clf.classifier_type == "decision_tree" else [])
    for name in methods:
        want = getattr(clf.model, name)(X)
        assert np.array_equal(getattr(clf, name)(X), want)
        assert clf.last_predict_stats == {'device': True, 'uncertified': uncertified}
        clf.last_predict_stats = None
        assert np.array_equal(getattr(clf, name)(torch.as_tensor(X, device="cuda:0")), want)
        assert clf.last_predict_stats == {'device': True, 'uncertified': uncertified}
