"""The fused MLP (csrc/mlp.hip) on the MI355X at the edges of its plan (tests/mlp_edge_cases.py):
training parity tensor by tensor against the restated reference, properties that hold bit for bit
by the kernel's summation order, and dsp_mlp_predict at nine shapes and two input scales.

Every bound comes from the fp64 and fp32 CPU runs of tests/mlp_reference.py and its MARGIN / FLOOR;
tests/test_mlp_edges_host.py shows on the CPU that the bounds catch the broken loops and that no
train-mode logit row is near a tie, which is why the hit counts are compared exactly here."""
import math

import numpy as np
import pytest
import torch

import mlp_edge_cases as E
import mlp_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ('params', 'm', 'v')


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def gpu_train(hidden, C, batch, X, y, perm, w0, p, lr=E.LR, seed=E.HASH_SEED):
    """One model through dsp_mlp_train from zero moments: dict of numpy arrays (params, m, v [P],
    steps, loss_hist, acc_hist [E])."""
    from src.pipeline import mlp_train
    params = _dev(np.asarray(w0, dtype=np.float32)[None], torch.float32)
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    steps = torch.zeros(1, dtype=torch.int64, device=DEV)
    loss, acc = mlp_train(_dev(X, torch.float32), _dev(y, torch.int32), hidden, C, _dev(perm, torch.int32), params, m, v,
                          steps, _dev(np.array([lr], dtype=np.float64), torch.float64),
                          _dev(np.array([seed], dtype=np.uint32).view(np.int32), torch.int32), batch, dropout=p)
    torch.cuda.synchronize()
    return dict(params=params.cpu().numpy()[0], m=m.cpu().numpy()[0], v=v.cpu().numpy()[0],
                steps=int(steps.cpu().numpy()[0]), loss_hist=loss.cpu().numpy()[0], acc_hist=acc.cpu().numpy()[0])


def gpu_predict(w, X, hidden, C, with_logits=True):
    from src.pipeline import mlp_predict
    pred, logits = mlp_predict(w, X, hidden, C, with_logits=with_logits)
    return pred.cpu().numpy(), None if logits is None else logits.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_bits(a, b, keys=KEYS + ('steps', 'loss_hist', 'acc_hist')):
    for k in keys:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def assert_hits(got, hits, N):
    """acc_hist is float32(hits / N) for the reference's hit count, and gives that count back."""
    for e, h in enumerate(hits):
        assert got['acc_hist'][e] == np.float32(int(h) / N), (e, got['acc_hist'][e] * N, h)
        assert round(float(got['acc_hist'][e]) * N) == int(h), e


# ---- parity ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,p", E.CASE_PS)
def test_edge_parity(name, p):
    """params, m and v of every tensor within MARGIN x (the fp32 CPU run's deviation from the fp64
    run in that tensor) + FLOOR of the fp64 run; loss_hist within the loss bound of
    test_gpu_mlp.py; steps and the hit count of every epoch exact."""
    c = E.BY_NAME[name]
    X, y, perm, w0 = c.inputs()
    ref, ref32 = E.reference(name, p, torch.float64), E.reference(name, p, torch.float32)
    got = gpu_train(c.hidden, c.C, c.batch, X, y, perm, w0, p)
    assert got['steps'] == ref['steps'] == E.EPOCHS * c.n_batches
    names = R.tensor_names(c.dims)
    over = []
    for key in KEYS:
        dev = R.per_tensor_deviation(got[key], ref[key], c.dims)
        bound = E.bounds(name, p, key)
        raw = (bound - R.FLOOR) / R.MARGIN
        for n, d, r, b in zip(names, dev, raw, bound):
            print("%s p=%g %s %s: GPU deviation %.3g, fp32 CPU reference's %.3g, ratio %s, bound %.3g, ratio to bound %.3g"
                  % (name, p, key, n, d, r, "%.3g" % (d / r) if r > 0 else "-", b, d / b))
            if d > b:
                over.append((key, n, d, b))
    assert not over, over
    lbound = R.loss_bound(ref, ref32)
    ldev = float(np.max(np.abs(got['loss_hist'] - ref['loss_hist'])))
    print("%s p=%g loss_hist: GPU deviation %.3g, bound %.3g" % (name, p, ldev, lbound))
    assert np.isfinite(got['loss_hist']).all() and ldev <= lbound
    assert_hits(got, ref['hits'], c.N)


def test_null_hidden(monkeypatch):
    """n_hidden = 0 with hidden = NULL (the header allows it) gives the bits of the call with a pointer,
    in training and in predict."""
    from src import pipeline
    c = E.BY_NAME['linear_only']
    X, y, perm, w0 = c.inputs()
    a = gpu_train(c.hidden, c.C, c.batch, X, y, perm, w0, 0.0)
    pa, la = gpu_predict(a['params'], X, c.hidden, c.C)
    monkeypatch.setattr(pipeline, "_int_array", lambda values: (None, len(list(values))))
    b = gpu_train(c.hidden, c.C, c.batch, X, y, perm, w0, 0.0)
    pb, lb = gpu_predict(a['params'], X, c.hidden, c.C)
    assert_same_bits(a, b)
    assert np.array_equal(pa, pb) and np.array_equal(bits(la), bits(lb))
    assert not np.array_equal(a['params'], w0)


# ---- exact properties ----------------------------------------------------------------------------
def _embed(w_small, dims_small, dims_big):
    """The small model's packed vector inside the big model's, every other entry 0; and the index of
    each small entry in the big vector."""
    big, where = [], []
    off_s = off_b = 0
    for (i, o), (I, O) in zip(zip(dims_small[:-1], dims_small[1:]), zip(dims_big[:-1], dims_big[1:])):
        W = np.zeros((O, I), dtype=np.float32)
        W[:o, :i] = w_small[off_s:off_s + o * i].reshape(o, i)
        idx = (off_b + np.arange(O * I).reshape(O, I))[:o, :i]
        b = np.zeros(O, dtype=np.float32)
        b[:o] = w_small[off_s + o * i:off_s + o * i + o]
        where += [idx.reshape(-1), off_b + O * I + np.arange(o)]
        big += [W.reshape(-1), b]
        off_s += o * i + o
        off_b += O * I + O
    return np.concatenate(big), np.concatenate(where)


def test_zero_embedding():
    """15 -> [5, 17] -> 7 trained alone and embedded in 20 -> [16, 33] -> 7 (extra input columns,
    weights and biases 0): the shared entries of params, m, v and both histories have equal bits, every
    extra entry and its moments are 0.

    Forward: the extra terms are fmaf(x, 0, s) or fmaf(0, w, s) appended to the same sequential chain
    (forward_tiles adds 4 k at a time in index order and the chains start at +0, so s is never -0 and
    s + 0 * w = s); an extra unit's activation is relu(0 + 0) = 0, dropped or scaled it stays 0, and
    its derivative (activation > 0) is 0; the dropout hash of a shared unit depends on (row, unit)
    alone.  Backward: a dW element is one chain over the batch rows whatever tile owns it; the delta
    chains run over the outputs in index order and the extra outputs add fmaf(0, 0, s).  Update: Adam
    with g = 0 and m = v = 0 leaves m = v = 0 and w = 0 - step * (0 / 1e-8) = 0.  The embedding moves
    n4 (2 -> 4, 5 -> 9), NJ (1 -> 1, 2 -> 3) and in4 / out4 of every layer at once."""
    ds, db = R.layer_dims(15, [5, 17], 7), R.layer_dims(20, [16, 33], 7)
    _, _, _, batch, N = R.PARITY_SHAPES['odd_16']
    X, y, perm, w0 = R.make_inputs(15, [5, 17], 7, N, 1010)
    small = gpu_train([5, 17], 7, batch, X, y, perm, w0, 0.3)
    wb, where = _embed(w0, ds, db)
    Xb = np.zeros((N, 20), dtype=np.float32)
    Xb[:, :15] = X
    big = gpu_train([16, 33], 7, batch, Xb, y, perm, wb, 0.3)
    extra = np.ones(wb.shape[0], dtype=bool)
    extra[where] = False
    assert extra.sum() == wb.shape[0] - w0.shape[0] and not np.array_equal(small['params'], w0)
    for key in KEYS:
        assert np.array_equal(bits(big[key][where]), bits(small[key])), key
        assert np.all(big[key][extra] == 0), key
    assert_same_bits(small, big, ('steps', 'loss_hist', 'acc_hist'))


def _largest_batch(D, hidden, C):
    from src.pipeline import mlp_lds_bytes
    lo, hi = 1, 4097  # admitted, refused
    assert mlp_lds_bytes(D, hidden, C, lo) > 0 and mlp_lds_bytes(D, hidden, C, hi) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if mlp_lds_bytes(D, hidden, C, mid) > 0:
            lo = mid
        else:
            hi = mid
    return lo


def test_plan_size_is_invisible():
    """N = 7 rows at batch 7, batch 16 and the largest batch the LDS plan admits: the carve-up differs
    (every activation buffer is batch_size rows), the steps are the same 7 rows, and so is every bit."""
    D, hidden, C, _, N, X, y, perm, w0 = R.parity_inputs('n_below_batch')
    top = _largest_batch(D, hidden, C)
    assert top > 16
    runs = [gpu_train(hidden, C, b, X, y, perm, w0, 0.3) for b in (7, 16, top)]
    assert_same_bits(runs[0], runs[1])
    assert_same_bits(runs[0], runs[2])
    assert runs[0]['steps'] == R.PARITY_EPOCHS and not np.array_equal(runs[0]['params'], w0)


def _ce_bound(C, N, row_loss):
    """(C + N + 16) * 2^-24 * max(1, largest row loss).  The trainer's row loss is logf(sum_c expf(z_c - mx))
    - (z_y - mx) in float32: C additions into a sum in [1, C], each rounding it by at most 2^-24 of
    itself, which logf carries over as an absolute error; the batch loss is N more float32 additions
    of row losses and one division, each within 2^-24 of a value no larger than the largest row loss;
    16 covers what is left at an ulp or two each: the C expf (their errors average into the sum's
    relative error), logf, the two subtractions, the division and the float32 store of the history."""
    return (C + N + 16) * 2.0 ** -24 * max(1.0, float(np.max(row_loss)))


def _mean_ce(logits, y):
    z = logits.astype(np.float64)
    z = z - z.max(1, keepdims=True)
    row = np.log(np.exp(z).sum(1)) - z[np.arange(len(y)), y]
    return float(row.mean()), row


@pytest.mark.parametrize("name", ['tile_steps', 'max_plan', 'linear_only'])
def test_lr_zero_ties_trainer_to_predict(name):
    """lr = 0, one epoch, one batch of all rows, no dropout: Adam's step is w - 0 * (m / denom) = w, so the
    parameters keep their bits; the trainer's forward pass is then predict's (both run forward_tiles
    over the same chains), so its hit count is the number of rows where predict's label is y, and its
    loss is the mean cross entropy of predict's logits to within the float32 roundings of the sum
    (_ce_bound).  max_plan trains on its first 48 rows, the largest batch its plan admits."""
    c = E.BY_NAME[name]
    X, y, perm, w0 = c.inputs()
    N = min(c.N, _largest_batch(c.D, c.hidden, c.C))
    assert N == (48 if name == 'max_plan' else c.N)
    X, y = X[:N], y[:N]
    order = perm[:1][perm[:1] < N].reshape(1, N)
    got = gpu_train(c.hidden, c.C, N, X, y, order, w0, 0.0, lr=0.0)
    assert got['steps'] == 1
    assert np.array_equal(bits(got['params']), bits(w0))
    assert np.any(got['m']) and np.any(got['v'])  # the step ran: only its size was 0
    pred, logits = gpu_predict(w0, X, c.hidden, c.C)
    assert_hits(got, [int((pred == y).sum())], N)
    mean, row = _mean_ce(logits, y)
    bound = _ce_bound(c.C, N, row)
    print("%s: loss %.9g, cross entropy of predict's logits %.9g, difference %.3g, bound %.3g"
          % (name, got['loss_hist'][0], mean, abs(got['loss_hist'][0] - mean), bound))
    assert abs(float(got['loss_hist'][0]) - mean) <= bound


def test_clamps():
    """Labels -1, C and C + 5 act as 0, C - 1 and C - 1; perm entries -1, N and N + 1 as 0, N - 1 and
    N - 1: the bits of every output equal those of the run with the in-range values.  (mlp.hip clamps
    the perm entry before X and y are read through it, and the label before the softmax indexes the
    logits with it.)"""
    D, hidden, C, batch, N, X, y, perm, w0 = R.parity_inputs('odd_16')
    good = gpu_train(hidden, C, batch, X, y, perm, w0, 0.3)
    y2 = y.copy()
    lo, hi = np.flatnonzero(y == 0), np.flatnonzero(y == C - 1)
    y2[lo[0]], y2[hi[0]], y2[hi[1]] = -1, C, C + 5
    labels = gpu_train(hidden, C, batch, X, y2, perm, w0, 0.3)
    assert_same_bits(good, labels)
    perm2 = perm.copy()
    perm2[0][perm[0] == 0] = -1
    perm2[0][perm[0] == N - 1] = N
    perm2[1][perm[1] == N - 1] = N + 1
    assert (perm2 != perm).sum() == 3
    order = gpu_train(hidden, C, batch, X, y, perm2, w0, 0.3)
    assert_same_bits(good, order)
    both = gpu_train(hidden, C, batch, X, y2, perm2, w0, 0.3)
    assert_same_bits(good, both)


def test_dead_layer():
    """One hidden layer whose biases are -1e3: every activation is 0 and so is its derivative, so the
    gradient of every tensor but the last bias is 0 in every step: those tensors keep their bits and
    their m and v are exactly 0; the last bias follows the reference within its bound."""
    c = E.BY_NAME['rows_7']
    X, y, perm, w0 = c.inputs()
    w0 = w0.copy()
    parts = R.split_packed(w0, c.dims)
    parts[1][:] = -1e3
    kw = dict(seed=E.HASH_SEED, p=0.3)
    ref = R.train(w0, c.D, c.hidden, c.C, X, y, perm, c.batch, E.LR, **kw)
    ref32 = R.train(w0, c.D, c.hidden, c.C, X, y, perm, c.batch, E.LR, dtype=torch.float32, **kw)
    assert [bool(np.any(t)) for t in R.split_packed(ref['m'], c.dims)] == [False, False, False, True]
    got = gpu_train(c.hidden, c.C, c.batch, X, y, perm, w0, 0.3)
    for key in KEYS:
        g = R.split_packed(got[key], c.dims)
        for t, (new, old) in enumerate(zip(g[:3], parts[:3])):
            if key == 'params':
                assert np.array_equal(bits(new), bits(old)), t
            else:
                assert np.all(new == 0), (key, t)
        dev = R.per_tensor_deviation(got[key], ref[key], c.dims)[3]
        bound = R.bound_per_tensor(ref, ref32, c.dims, key)[3]
        print("dead layer, last bias %s: GPU deviation %.3g, bound %.3g" % (key, dev, bound))
        assert dev <= bound, key
    assert not np.array_equal(R.split_packed(got['params'], c.dims)[3], parts[3])
    assert float(np.max(np.abs(got['loss_hist'] - ref['loss_hist']))) <= R.loss_bound(ref, ref32)
    assert_hits(got, ref['hits'], c.N)


def test_ties_take_the_first_index():
    """Last-layer weights 0 and equal biases: every logit of every row is equal, so predict's label and
    the trainer's argmax are index 0 (torch.max's choice); with lr = 0 the accuracy is the share of
    y == 0 in every epoch and the loss is log C within _ce_bound."""
    D, hidden, C, batch, N, X, y, perm, w0 = R.parity_inputs('odd_16')
    w0 = w0.copy()
    parts = R.split_packed(w0, R.layer_dims(D, hidden, C))
    parts[-2][:] = 0.0
    parts[-1][:] = 0.25
    pred, logits = gpu_predict(w0, X, hidden, C)
    assert np.all(logits == np.float32(0.25)) and np.all(pred == 0)
    got = gpu_train(hidden, C, batch, X, y, perm, w0, 0.3, lr=0.0)
    assert np.array_equal(bits(got['params']), bits(w0))
    assert_hits(got, [int((y == 0).sum())] * R.PARITY_EPOCHS, N)
    bound = _ce_bound(C, batch, [math.log(C)])
    assert np.max(np.abs(got['loss_hist'].astype(np.float64) - math.log(C))) <= bound


def test_one_class():
    """C = 1 is inside the plan: the softmax of one logit is 1, so the loss is exactly 0, every gradient
    is 0 and the parameters keep their bits at lr = 1e-3; every label is 0 and every row a hit."""
    D, hidden, C, N, batch = 15, [64, 64, 32], 1, 21, 8
    X, y, perm, w0 = R.make_inputs(D, hidden, C, N, 1011)
    assert not y.any()
    got = gpu_train(hidden, C, batch, X, y, perm, w0, 0.3)
    assert got['steps'] == R.PARITY_EPOCHS * 3
    assert np.array_equal(bits(got['params']), bits(w0))
    assert np.all(got['m'] == 0) and np.all(got['v'] == 0)
    assert np.array_equal(bits(got['loss_hist']), np.zeros(R.PARITY_EPOCHS, dtype=np.uint32))
    assert np.all(got['acc_hist'] == 1.0)
    pred, logits = gpu_predict(w0, X, hidden, C)
    assert np.all(pred == 0) and logits.shape == (N, 1)


# ---- predict -------------------------------------------------------------------------------------
PREDICT_RUNS = [(s, E.PREDICT_ROWS) for s, _ in E.PREDICT_SHAPES] + [(s, nq) for s in E.PREDICT_DEEPEST for nq in (1, 65)]


@pytest.mark.parametrize("shape,nq", PREDICT_RUNS, ids=lambda v: E.predict_id(v) if isinstance(v, tuple) else str(v))
def test_predict_edges(shape, nq):
    """Logits within PREDICT_MARGIN x (fp32 CPU forward's deviation) + FLOOR of the fp64 reference at
    input scales 1 and 100, labels equal on every row that is not excluded, and the call without a
    logits buffer gives the same labels."""
    D, hidden, C = shape
    for scale in E.PREDICT_SCALES:
        w, X = E.predict_inputs(shape, scale)
        l64, tol, excluded = E.predict_reference(shape, scale)
        pred, logits = gpu_predict(w, X[:nq], list(hidden), C)
        assert logits.shape == (nq, C) and pred.shape == (nq,)
        dev = float(np.max(np.abs(logits - l64[:nq])))
        print("predict %s x%g nq=%d: logit deviation %.3g, tolerance %.3g, excluded rows %d"
              % (E.predict_id(shape), scale, nq, dev, tol, excluded[:nq].sum()))
        assert dev <= tol
        keep = ~excluded[:nq]
        assert np.array_equal(pred[keep], l64[:nq].argmax(1)[keep])
        pred2, none = gpu_predict(w, X[:nq], list(hidden), C, with_logits=False)
        assert none is None and np.array_equal(pred2, pred)
