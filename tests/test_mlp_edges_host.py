"""CPU checks behind the MLP edge tests (tests/test_gpu_mlp_edges.py): the inputs of the existing
parity cases are pinned, the per-tensor bounds catch each broken loop on every edge case, no
train-mode logit row of any case is near a tie (which is what lets the GPU test compare hit counts
exactly), every tensor of every case moves, the predict inputs are fair, and the host side of the
entry points (LDS plan, parameter count, early returns) answers as the header says."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import mlp_edge_cases as E
import mlp_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_parity_inputs.npz")


@pytest.mark.parametrize("name", ['config_108', 'n_below_batch', 'odd_16', 'tiny_4'])
def test_parity_inputs_are_pinned(name):
    """parity_inputs(name) is bit for bit what it was when the seed was the name's rank among the four:
    shape, SHA-256 and the first four values of X, y, perm and the initial weights."""
    pins = np.load(GOLDEN)
    assert R.PARITY_DATA_SEEDS == {'config_108': 11, 'n_below_batch': 12, 'odd_16': 13, 'tiny_4': 14}
    for field, a in zip(('X', 'y', 'perm', 'packed0'), R.parity_inputs(name)[5:]):
        a = np.ascontiguousarray(a)
        key = "%s/%s/" % (name, field)
        assert list(a.shape) == list(pins[key + "shape"]), key
        assert a.dtype == pins[key + "head"].dtype, key
        assert np.array_equal(a.reshape(-1)[:4], pins[key + "head"]), key
        assert hashlib.sha256(a.tobytes()).digest() == pins[key + "sha256"].tobytes(), key


def test_split_packed_is_state_dict_order():
    dims = R.layer_dims(15, [33, 17], 7)
    net = R.build_sequential(15, [33, 17], 7)
    packed = np.concatenate([t.detach().numpy().reshape(-1) for t in net.state_dict().values()])
    parts = R.split_packed(packed, dims)
    assert R.tensor_names(dims) == ['W0', 'b0', 'W1', 'b1', 'W2', 'b2']
    for part, t in zip(parts, net.state_dict().values()):
        assert np.array_equal(part, t.numpy().reshape(-1))
    assert R.split_packed(np.zeros(15 * 10 + 10), R.layer_dims(15, [], 10))[1].shape == (10,)
    # a deviation in one tensor shows in that tensor alone
    other = packed.copy()
    other[15 * 33 + 2] += 0.5  # b0[2]
    assert list(R.per_tensor_deviation(packed, other, dims) > 0) == [False, True, False, False, False, False]


def test_edge_table():
    """The table's claims about itself: names, the short last batches, the rows % 4 of the row clamps,
    the NJ of every layer of tile_steps."""
    assert [c.name for c in E.CASES] == ['linear_only', 'max_plan', 'tile_steps', 'batch_1', 'rows_5', 'rows_7',
                                         'rows_6', 'width_one', 'heavy_dropout', 'saturated']
    seeds = [c.data_seed for c in E.CASES if c.like is None]
    assert len(set(seeds)) == len(seeds)
    last = {c.name: c.N - (c.n_batches - 1) * c.batch for c in E.CASES}
    assert (last['max_plan'], last['tile_steps'], last['rows_5'], last['rows_7'], last['rows_6']) == (4, 3, 3, 3, 2)
    assert [E.BY_NAME[n].batch % 4 for n in ('rows_5', 'rows_6', 'rows_7')] == [1, 2, 3]
    nj = [-(-((w + 3) // 4 * 4) // 16) for w in E.BY_NAME['tile_steps'].dims[1:]]
    assert nj == [1, 2, 3, 4, 3]
    for n in ('heavy_dropout', 'saturated'):
        X, y, perm, w0 = E.BY_NAME[n].inputs()
        Xo, yo, permo, wo = R.parity_inputs('odd_16')[5:]
        assert np.array_equal(y, yo) and np.array_equal(perm, permo) and np.array_equal(w0, wo)
        assert np.array_equal(X, Xo * np.float32(E.BY_NAME[n].x_scale))
    # saturated: batch losses past the 89 at which an unshifted expf overflows
    for p in E.BY_NAME['saturated'].ps:
        assert E.reference('saturated', p)['loss_hist'].min() > 89.0
    assert [round(R.drop_threshold(p)[1], 2) for p in E.BY_NAME['heavy_dropout'].ps] == [10.0, 100.0, 1000.0]


@pytest.mark.parametrize("name,p", E.CASE_PS)
def test_per_tensor_bounds_catch_broken_variants(name, p):
    """Each broken loop that differs from the right one by construction on this case moves at least
    one tensor by more than 10x that tensor's bound."""
    case = E.BY_NAME[name]
    good = E.reference(name, p)['params']
    bound = E.bounds(name, p, 'params')
    for variant in E.variants_for(case, p):
        bad = E.reference(name, p, torch.float64, variant)['params']
        ratio = R.per_tensor_deviation(good, bad, case.dims) / bound
        print("%s %s p=%g: largest ratio %.3g in %s" % (variant, name, p, ratio.max(),
                                                      R.tensor_names(case.dims)[int(ratio.argmax())]))
        assert ratio.max() > 10, (variant, ratio)


def test_variants_apply_where_they_differ():
    got = {c.name: E.variants_for(c, c.ps[1]) for c in E.CASES}
    assert got['linear_only'] == ['no_bias_correction', 'sum_short_batch']  # no hidden layer: no keep scale
    assert got['batch_1'] == got['width_one'] == ['no_bias_correction', 'no_keep_scale']
    assert got['heavy_dropout'] == got['saturated'] == ['no_bias_correction', 'no_keep_scale']  # last batch: 1 row
    # p = 0.999 drops the whole last hidden layer in every step: the scale multiplies nothing that is kept
    assert E.variants_for(E.BY_NAME['heavy_dropout'], 0.999) == ['no_bias_correction']
    for n in ('max_plan', 'tile_steps', 'rows_5', 'rows_6', 'rows_7'):
        assert got[n] == ['no_bias_correction', 'no_keep_scale', 'sum_short_batch'], n
    assert E.variants_for(E.BY_NAME['max_plan'], 0.0) == ['no_bias_correction', 'sum_short_batch']


def _near_tie_rows(ref64, ref32):
    thr, cnt = R.near_ties(ref64, ref32)
    assert (thr > 0).all() and len(thr) == E.EPOCHS
    return int(cnt.sum())


@pytest.mark.parametrize("name,p", E.CASE_PS)
def test_no_edge_row_is_near_a_tie(name, p):
    assert _near_tie_rows(E.reference(name, p), E.reference(name, p, torch.float32)) == 0


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("name", list(R.PARITY_SHAPES))
def test_no_parity_row_is_near_a_tie(name, p):
    assert _near_tie_rows(R.parity_reference(name, p), R.parity_reference(name, p, torch.float32)) == 0


def test_near_tie_count_sees_a_tie():
    """The count is not vacuous: rows with a top-2 gap under the threshold are counted, others not."""
    l64 = [[np.array([[0.0, 1.0, 1.0 + 1e-9], [0.0, 5.0, 1.0]])]]
    l32 = [[np.array([[0.0, 1.0, 1.0], [0.0, 5.0, 1.0]])]]
    thr, cnt = R.near_ties(dict(logits=l64), dict(logits=l32))
    assert thr[0] == 2 * (R.MARGIN * np.abs(l64[0][0] - l32[0][0]).max() + R.FLOOR) and list(cnt) == [1]


@pytest.mark.parametrize("name,p", E.CASE_PS)
def test_every_tensor_moves(name, p):
    """No tensor of the fp64 run has an all-zero m, except those the case names as dead."""
    case = E.BY_NAME[name]
    m = R.split_packed(E.reference(name, p)['m'], case.dims)
    dead = tuple(n for n, t in zip(R.tensor_names(case.dims), m) if not np.any(t))
    assert dead == tuple(case.dead.get(p, ())), dead


@pytest.mark.parametrize("shape", [s for s, _ in E.PREDICT_SHAPES], ids=E.predict_id)
def test_predict_inputs_are_fair(shape):
    """At least two classes predicted in fp64 (C >= 2) and at most 1 % of the rows excluded."""
    for scale in E.PREDICT_SCALES:
        l64, tol, excluded = E.predict_reference(shape, scale)
        assert l64.shape == (E.PREDICT_ROWS, shape[2]) and np.isfinite(l64).all()
        assert excluded.mean() <= 0.01, (scale, excluded.mean())
        if shape[2] >= 2:
            assert len(np.unique(l64.argmax(1))) >= 2, scale


# ---- the host side of the entry points ----------------------------------------------------------
def test_lds_plan():
    from src import _hip
    from src.pipeline import mlp_lds_bytes, mlp_param_count
    lib = _hip.load_library()
    assert mlp_lds_bytes(15, [64, 64, 32], 10, 108) == 115744
    assert mlp_lds_bytes(15, [64, 64, 32], 64, 108) == 145904
    c = E.BY_NAME['max_plan']
    assert mlp_lds_bytes(c.D, c.hidden, c.C, 48) == 4 * 40612
    assert mlp_lds_bytes(c.D, c.hidden, c.C, 49) == 0  # 41 004 words of 40 960
    for case in E.CASES:
        assert mlp_lds_bytes(case.D, case.hidden, case.C, case.batch) > 0, case
    for D, hidden, C in [(c.D, c.hidden, c.C), (15, [64, 64, 32], 10), (1, [1, 1], 2), (15, [], 10)]:
        prev, b = 0, 1
        while True:
            got = mlp_lds_bytes(D, hidden, C, b)
            if got == 0:
                break
            assert got >= prev and got <= 160 * 1024, (D, hidden, C, b)
            prev, b = got, b + 1
        assert b > 1 and all(mlp_lds_bytes(D, hidden, C, b + k) == 0 for k in (1, 2, 100))  # no second admitted range
    # n_hidden = 0 with a NULL hidden
    assert lib.dsp_mlp_lds_bytes(15, 0, None, 10, 16) == mlp_lds_bytes(15, [], 10, 16) > 0
    assert lib.dsp_mlp_lds_bytes(15, 1, None, 10, 16) == 0
    assert lib.dsp_mlp_param_count(15, 0, None, 10) == mlp_param_count(15, [], 10) == 15 * 10 + 10
    assert lib.dsp_mlp_param_count(1, 0, None, 1) == 2
    assert mlp_param_count(64, [64] * 4, 64) == 5 * (64 * 64 + 64)


def test_early_returns():
    """n_epochs = 0 returns DSP_OK before any launch; a stride that is set but too small is refused.
    The buffer is never read: both answers come from the host checks."""
    from src import _hip
    lib = _hip.load_library()
    buf = ctypes.create_string_buffer(64)
    q = ctypes.cast(buf, ctypes.c_void_p)
    arr = (ctypes.c_int * 2)(33, 17)
    N, D, E_ = 10, 15, 2

    def tr(n_epochs=E_, x_stride=0, y_stride=0, perm_stride=0, n_hidden=2, hidden=arr):
        return lib.dsp_mlp_train(q, q, N, x_stride, y_stride, D, n_hidden, hidden, 7, 1, n_epochs, 16, q, perm_stride, q,
                                 q, q, q, q, q, 0, 1.0, q, q, None)
    assert tr(n_epochs=0) == _hip.DSP_OK
    assert tr(n_epochs=0, n_hidden=0, hidden=None) == _hip.DSP_OK
    assert tr(n_epochs=-1) == _hip.DSP_ERR_ARGS
    assert tr(n_epochs=0, n_hidden=2, hidden=None) == _hip.DSP_ERR_ARGS
    assert tr(n_epochs=0, x_stride=N * D, y_stride=N, perm_stride=E_ * N) == _hip.DSP_OK
    assert tr(x_stride=N * D - 1) == _hip.DSP_ERR_ARGS
    assert tr(y_stride=N - 1) == _hip.DSP_ERR_ARGS
    assert tr(perm_stride=E_ * N - 1) == _hip.DSP_ERR_ARGS
    assert tr(x_stride=1) == tr(y_stride=1) == tr(perm_stride=1) == _hip.DSP_ERR_ARGS
