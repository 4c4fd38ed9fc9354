"""Edge cases of the fused MLP (csrc/mlp.hip): named, seeded training runs and predict shapes at the
limits of the LDS plan, on either side of every forward_tiles<NJ> instantiation, at every rows % 4
of the row clamps, and at the numeric ends of dropout and of the cross entropy (a plain helper
module like tests/knn_edge_cases.py: no test, no fixture; it never touches the device library).

Training cases use the recipe of mlp_reference.make_inputs (labels arange(N) % C shuffled, Gaussian
class centres, three shuffle orders, nn.Linear default init) with their own data seed, 3 epochs at
lr = 1e-3, dropout hash seed 1234 and p in {0, 0.3} unless the row says otherwise:

  linear_only    15 -> 10, batch 16, N 40          n_hidden = 0, hidden NULL, no delta stage
  max_plan       64 -> 64 x 4 -> 64, 48, 100       every limit at once; 48 is the largest batch
                                                   inside 160 KiB (22 080 + 48 * 384 + 2 * 48 + 4 =
                                                   40 612 words of 40 960; 41 004 at 49); last batch 4
  tile_steps     7 -> 16, 17, 48, 49 -> 33, 6, 21  NJ = 1, 2, 3, 4, 3; last batch 3 rows
  batch_1        15 -> 33, 17 -> 7, 1, 6           one row per step
  rows_5/7/6     4 -> 20 -> 3                      rows % 4 = 1, 3, 2; last batches 3, 3, 2
  width_one      1 -> 1, 1 -> 2, 1, 5              D, widths and batch all 1
  heavy_dropout  odd_16's inputs, p = 0.9, 0.99,   rows and whole layers dropped, keep_scale 10, 100,
                 0.999                             1000
  saturated      odd_16's inputs, X * 3000         batch losses of 300 to 800: an unshifted expf overflows

``dead`` names, per p, the tensors whose Adam m stays all zero in the fp64 reference because the
case's definition says so (tests/test_mlp_edges_host.py holds the reference to exactly that list).
"""
import numpy as np
import torch

import mlp_reference as R

EPOCHS = R.PARITY_EPOCHS
LR = R.PARITY_LR
HASH_SEED = R.PARITY_SEED


class MlpCase:
    def __init__(self, name, D, hidden, C, batch, N, data_seed=None, init_seed=7, ps=(0.0, 0.3), like=None,
                 x_scale=1.0, dead=None):
        self.name, self.D, self.hidden, self.C, self.batch, self.N = name, D, list(hidden), C, batch, N
        self.data_seed, self.init_seed, self.ps, self.like, self.x_scale = data_seed, init_seed, tuple(ps), like, x_scale
        self.dead = dead or {}
        self.dims = R.layer_dims(D, hidden, C)

    def inputs(self):
        """(X float32 [N, D], y int32 [N], perm int32 [E, N], packed0 float32)"""
        if self.like is not None:
            X, y, perm, w0 = R.parity_inputs(self.like)[5:]
            return (X * np.float32(self.x_scale)).astype(np.float32), y, perm, w0
        return R.make_inputs(self.D, self.hidden, self.C, self.N, self.data_seed, self.init_seed, EPOCHS)

    @property
    def n_batches(self):
        return -(-self.N // self.batch)

    @property
    def short_batch(self):
        """rows of the last batch when it is shorter than the others, else 0"""
        r = self.N % self.batch
        return r if self.N > self.batch else 0

    def __repr__(self):
        return "MlpCase(%s)" % self.name


_ODD = R.PARITY_SHAPES['odd_16']
CASES = [
    MlpCase('linear_only', 15, [], 10, 16, 40, 1000),
    MlpCase('max_plan', 64, [64, 64, 64, 64], 64, 48, 100, 1001),
    MlpCase('tile_steps', 7, [16, 17, 48, 49], 33, 6, 21, 1003),
    MlpCase('batch_1', 15, [33, 17], 7, 1, 6, 1004),
    MlpCase('rows_5', 4, [20], 3, 5, 18, 1005),
    MlpCase('rows_7', 4, [20], 3, 7, 17, 1006),
    MlpCase('rows_6', 4, [20], 3, 6, 20, 1007),
    # data and init seed chosen by tests/test_mlp_edges_host.py's conditions (init seed 7 leaves the
    # first unit dead): every tensor moves at both p and no step's logit row is near a tie
    MlpCase('width_one', 1, [1, 1], 2, 1, 5, 1008, init_seed=8),
    # at 0.999 no unit of the last hidden layer survives any step, so only the last bias ever moves; 0.99
    # (keep_scale 100) is the largest of the three at which kept units reach the logits
    MlpCase('heavy_dropout', *_ODD, like='odd_16', ps=(0.9, 0.99, 0.999),
            dead={0.99: ('W0', 'b0', 'W1'), 0.999: ('W0', 'b0', 'W1', 'b1', 'W2')}),
    MlpCase('saturated', *_ODD, like='odd_16', x_scale=3000.0),
]
BY_NAME = {c.name: c for c in CASES}
CASE_PS = [(c.name, p) for c in CASES for p in c.ps]

_CACHE = {}


def reference(name, p, dtype=torch.float64, variant=None):
    """mlp_reference.train() on the case's inputs, once per (case, p, precision, variant)."""
    key = (name, p, dtype, variant)
    if key not in _CACHE:
        c = BY_NAME[name]
        X, y, perm, w0 = c.inputs()
        _CACHE[key] = R.train(w0, c.D, c.hidden, c.C, X, y, perm, c.batch, LR, seed=HASH_SEED, p=p, dtype=dtype,
                              variant=variant, keep_logits=variant is None)
    return _CACHE[key]


def bounds(name, p, key):
    return R.bound_per_tensor(reference(name, p, torch.float64), reference(name, p, torch.float32),
                              BY_NAME[name].dims, key)


def variants_for(case, p):
    """The broken loops that differ from the right one by construction on this case (the reasons are
    with SENSITIVITY in tests/test_mlp_host.py)."""
    out = ['no_bias_correction']
    last_w = 'W%d' % len(case.hidden)
    if p > 0 and case.hidden and last_w not in case.dead.get(p, ()):  # no kept unit ever reaches the logits: no scale to miss
        out.append('no_keep_scale')
    if case.short_batch > 1:
        out.append('sum_short_batch')
    return out


# ---- predict -----------------------------------------------------------------------------------
PREDICT_ROWS = 200
PREDICT_SCALES = (1.0, 100.0)
# (D, hidden, C): init_packed seed.  The seed is the first from 7 upward at which the fp64 labels of
# both scales hold two classes or more and at most 1 % of the rows are excluded (host test).
PREDICT_SHAPES = [
    ((1, (), 2), 7),
    ((1, (1,), 2), 8),
    ((64, (), 64), 7),
    ((15, (), 10), 7),
    ((64, (64, 64, 64, 64), 64), 7),
    ((7, (16, 17, 48, 49), 33), 7),
    ((4, (4, 4, 4, 4), 4), 25),
    ((63, (1, 64), 3), 15),
    ((15, (64, 64, 32), 1), 7),
]
PREDICT_DEEPEST = [(64, (64, 64, 64, 64), 64), (7, (16, 17, 48, 49), 33)]  # also at Nq = 1 and 65


def predict_id(shape):
    D, hidden, C = shape
    return "%d-%s-%d" % (D, "x".join(map(str, hidden)) or "none", C)


def predict_inputs(shape, scale):
    """(packed weights float32, X float32 [200, D] = scale x normal rows)"""
    D, hidden, C = shape
    seed = dict(PREDICT_SHAPES)[shape]
    idx = [s for s, _ in PREDICT_SHAPES].index(shape)
    rng = np.random.default_rng(2000 + idx)
    X = (scale * rng.normal(size=(PREDICT_ROWS, D))).astype(np.float32)
    return R.init_packed(D, list(hidden), C, seed=seed), X


def predict_reference(shape, scale):
    """(logits64, tolerance, excluded rows) as mlp_reference.predict_reference defines them."""
    key = ('predict', shape, scale)
    if key not in _CACHE:
        D, hidden, C = shape
        w, X = predict_inputs(shape, scale)
        l64 = R.predict_logits(w, D, list(hidden), C, X, torch.float64)
        l32 = R.predict_logits(w, D, list(hidden), C, X, torch.float32)
        tol = R.PREDICT_MARGIN * float(np.max(np.abs(l64 - l32))) + R.FLOOR
        if C > 1:
            top = np.sort(l64, axis=1)
            excluded = (top[:, -1] - top[:, -2]) < 2 * tol
        else:
            excluded = np.zeros(PREDICT_ROWS, dtype=bool)
        _CACHE[key] = (l64, tol, excluded)
    return _CACHE[key]
