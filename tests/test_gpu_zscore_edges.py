"""The z-score kernels against numpy itself at the boundaries of their tiling
(tests/zscore_edge_cases.py): dsp_zscore_fit equals np.mean / np.std over axis 0 (std 0 -> 1) and
dsp_zscore_apply equals (X - mean) / std, bit for bit, out of place and in place."""
import numpy as np
import pytest

import zscore_edge_cases as zc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    """[(name, X, mean, std, Xn)] with numpy's own results, computed once."""
    out = []
    for name, X in zc.matrices():
        mean, std = np.mean(X, axis=0), np.std(X, axis=0)
        std = np.where(std == 0, 1.0, std)
        out.append((name, X, mean, std, (X - mean) / std))
    return out


def _apply_in_place(X, mean, std):
    """dsp_zscore_apply with out aliasing X (include/dsp_audiorec.h allows it)."""
    import torch
    from src import _hip
    d = _hip.require_device()
    x = torch.as_tensor(X.copy()).to(d)
    rc = _hip.lib().dsp_zscore_apply(_hip.ptr(x), x.shape[0], x.shape[1], _hip.ptr(mean), _hip.ptr(std), _hip.ptr(x),
                                     _hip.stream_handle(d))
    _hip.check(rc, "dsp_zscore_apply")
    return x.cpu().numpy()


def _check(selected):
    from src.pipeline import zscore_apply, zscore_fit
    bad = []
    for name, X, mean, std, Xn in selected:
        m, s = zscore_fit(X)
        wrong = [w for w, a, b in (("mean", m.cpu().numpy(), mean), ("std", s.cpu().numpy(), std),
                                   ("apply", zscore_apply(X, m, s).cpu().numpy(), Xn),
                                   ("in place", _apply_in_place(X, m, s), Xn)) if not np.array_equal(a, b)]
        if wrong:
            bad.append("%s: %s" % (name, ", ".join(wrong)))
    assert not bad, "%d of %d matrices:\n%s" % (len(bad), len(selected), "\n".join(bad))


@pytest.mark.parametrize("D", zc.DS)
def test_zscore_shapes(cases, D):
    sel = [c for c in cases if c[0].startswith("plain_") and c[1].shape[1] == D]
    assert len(sel) == len(zc.NS)
    _check(sel)


def test_zscore_constant_columns_and_offsets(cases):
    sel = [c for c in cases if not c[0].startswith("plain_")]
    assert len(sel) == 3 * len(zc.SPECIAL_SHAPES) + len(zc.LONG_COLUMNS)
    # the ordinary constant column really has std 0 in numpy (-> 1)
    for name, X, mean, std, Xn in sel:
        if name.startswith("constant_column"):
            assert std[X.shape[1] // 2] == 1.0 and (Xn[:, X.shape[1] // 2] == 0).all()
    _check(sel)
