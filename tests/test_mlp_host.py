"""CPU checks of the MLP feature: the restated reference (tests/mlp_reference.py) against torch's own
modules, the dropout hash, the sensitivity of the GPU comparison's tolerance, the new exports."""
import numpy as np
import pytest
import torch

import mlp_reference as R


def test_reference_equals_torch_module_loop():
    """Dropout off: the fp32 reference is bit-equal to an nn.Sequential built the same way and
    stepped with the same batches as the reference project's loop (zero_grad / backward / step)."""
    D, hidden, C, batch, N, X, y, perm, w0 = R.parity_inputs('odd_16')
    net = R.build_sequential(D, hidden, C)
    sd = net.state_dict()
    for t, src in zip(sd.values(), R.unpack(w0, R.layer_dims(D, hidden, C), torch.float32)):
        t.copy_(src)
    opt = torch.optim.Adam(net.parameters(), lr=R.PARITY_LR)
    crit = torch.nn.CrossEntropyLoss()
    Xt, yt = torch.FloatTensor(X), torch.LongTensor(y.astype(np.int64))
    net.eval()  # no dropout; ReLU and Linear are the same in both modes
    losses = []
    for e in range(perm.shape[0]):
        tot, nb = 0.0, 0
        for lo in range(0, N, batch):
            idx = torch.as_tensor(perm[e, lo:lo + batch].astype(np.int64))
            out = net(Xt[idx])
            loss = crit(out, yt[idx])
            opt.zero_grad()
            loss.backward()
            opt.step()
            tot += loss.item()
            nb += 1
        losses.append(tot / nb)
    ref = R.parity_reference('odd_16', 0.0, torch.float32)
    mine = np.concatenate([t.detach().numpy().reshape(-1) for t in net.state_dict().values()])
    assert np.array_equal(mine, ref['params'])
    assert losses == list(ref['loss_hist'])


def test_hash_keep_share():
    """>= 1e6 draws at p = 0.3: the keep share within 5 sigma of 0.7, overall and per layer and per
    step over 100 steps; masks of consecutive steps differ."""
    p, rows, width, steps, layers = 0.3, 108, 64, 100, 3
    sig = lambda n: 5 * np.sqrt(0.3 * 0.7 / n)
    total, prev = 0, None
    per_layer = np.zeros(layers)
    for s in range(steps):
        kept = 0
        for l in range(layers):
            m = R.keep_mask(R.PARITY_SEED, s, l, rows, width, p)
            per_layer[l] += m.sum()
            kept += m.sum()
            if l == 0:
                assert prev is None or not np.array_equal(m, prev)
                assert 0.2 < (m != prev).mean() < 0.65 if prev is not None else True  # 2 * 0.3 * 0.7 = 0.42
                prev = m
        n = layers * rows * width
        assert abs(kept / n - 0.7) < sig(n), (s, kept / n)
        total += kept
    n_all = steps * layers * rows * width
    assert n_all >= 1e6
    assert abs(total / n_all - 0.7) < sig(n_all)
    for l in range(layers):
        assert abs(per_layer[l] / (n_all / layers) - 0.7) < sig(n_all / layers), l
    # different seeds and the high word of the step change the stream
    a = R.dropout_hash(1, 5, 0, 16, 16)
    assert not np.array_equal(a, R.dropout_hash(2, 5, 0, 16, 16))
    assert not np.array_equal(a, R.dropout_hash(1, 5 + (1 << 32), 0, 16, 16))
    assert R.keep_mask(1, 5, 0, 16, 16, 0.0).all()  # threshold 0: nothing is dropped


# where each broken variant differs from the right loop by construction: the keep scale needs
# dropout; a summed short batch needs a short batch of more than one row next to full ones (with a
# single batch per epoch Adam's step is invariant to the gradient's scale, and a one-row batch's sum
# is its mean)
SENSITIVITY = [('no_bias_correction', name, p) for name in R.PARITY_SHAPES for p in (0.0, 0.3)] + \
              [('no_keep_scale', name, 0.3) for name in R.PARITY_SHAPES] + \
              [('sum_short_batch', name, p) for name in ('config_108', 'tiny_4') for p in (0.0, 0.3)]


@pytest.mark.parametrize("variant,name,p", SENSITIVITY)
def test_tolerance_catches_broken_variants(variant, name, p):
    """Each broken loop moves the parameters by at least 10x the bound the GPU comparison uses."""
    good = R.parity_reference(name, p, torch.float64)['params']
    bad = R.parity_reference(name, p, torch.float64, variant)['params']
    bound = R.parity_bound(name, p)
    dev = float(np.max(np.abs(good - bad)))
    print("%s %s p=%.1f: deviation %.3g, bound %.3g, ratio %.3g" % (variant, name, p, dev, bound, dev / bound))
    assert dev > 10 * bound


def test_predict_exclusion_cap():
    """At most 1 % of the predict rows have an fp64 top-2 logit gap under the exclusion threshold."""
    l64, tol, excluded = R.predict_reference()
    assert l64.shape == (R.PREDICT_N, 10)
    assert excluded.mean() <= 0.01, excluded.mean()
    assert len(np.unique(l64.argmax(1))) > 1  # the trained weights do not predict one class only


def test_create_classifier_mlp_without_gpu():
    from src import _hip
    from src.models import MLPTrainer, create_classifier
    clf = create_classifier('mlp', input_size=15, hidden_layers=[64, 32], num_classes=4, seed=1)
    assert isinstance(clf, MLPTrainer) and clf.epochs == 100 and clf.batch_size == 16
    assert clf.train_losses == [] and clf.train_accuracies == []
    net = clf.model
    assert [type(m).__name__ for m in net] == ['Linear', 'ReLU', 'Dropout', 'Linear', 'ReLU', 'Dropout', 'Linear']
    assert net[2].p == 0.3
    # nn.Linear default init, reproducible from the seed without touching the global RNG
    state = torch.random.get_rng_state()
    again = create_classifier('mlp', input_size=15, hidden_layers=[64, 32], num_classes=4, seed=1)
    assert torch.equal(state, torch.random.get_rng_state())
    assert torch.equal(again._params, clf._params)
    assert np.array_equal(clf._params.numpy(), R.init_packed(15, [64, 32], 4, seed=1))
    with pytest.raises(NotImplementedError, match="input_size.*hidden_layers.*num_classes"):
        create_classifier('mlp')
    with pytest.raises(ValueError):
        create_classifier('mlp', input_size=3, hidden_layers=[4], num_classes=2, backend='cpu')
    if not torch.cuda.is_available():
        with pytest.raises(_hip.HipError):
            clf.fit(np.zeros((4, 15)), np.zeros(4, dtype=np.int64), verbose=False)


def test_abi_exports_and_lds_plan():
    import ctypes
    from src import _hip
    from src.pipeline import mlp_lds_bytes, mlp_param_count
    lib = _hip.load_library()
    for name in ("dsp_mlp_lds_bytes", "dsp_mlp_param_count", "dsp_mlp_train", "dsp_mlp_predict",
                 "dsp_mlp_dropout_mask"):
        assert hasattr(lib, name) and name in _hip.EXPORTS, name
    assert lib.dsp_abi_version() == 6  # new symbols only: the version stays
    # the two configurations that must be inside the fused plan
    assert 0 < mlp_lds_bytes(15, [64, 64, 32], 10, 108) <= 160 * 1024
    assert 0 < mlp_lds_bytes(15, [64, 64, 32], 64, 108) <= 160 * 1024
    assert 0 < mlp_lds_bytes(15, [64, 32], 10, 16) <= 160 * 1024
    for name, (D, hidden, C, batch, N) in R.PARITY_SHAPES.items():
        assert mlp_lds_bytes(D, hidden, C, batch) > 0, name
    # outside: wide inputs (the sequence method), wide layers, too many layers, a batch beyond LDS
    assert mlp_lds_bytes(300, [64, 32], 10, 16) == 0
    assert mlp_lds_bytes(15, [128], 10, 16) == 0
    assert mlp_lds_bytes(15, [8] * 5, 10, 16) == 0
    assert mlp_lds_bytes(15, [64, 64, 32], 10, 4096) == 0
    assert mlp_lds_bytes(15, [64], 0, 16) == 0 and mlp_lds_bytes(15, [64], 10, 0) == 0
    arr = (ctypes.c_int * 3)(64, 64, 32)
    assert lib.dsp_mlp_param_count(15, 3, arr, 10) == mlp_param_count(15, [64, 64, 32], 10) == 7594
    # argument errors come back from the host, before any launch
    buf = ctypes.create_string_buffer(64)
    q = ctypes.cast(buf, ctypes.c_void_p)
    tr = lambda D=15, N=10, X=q: lib.dsp_mlp_train(X, q, N, 0, 0, D, 3, arr, 10, 1, 1, 16, q, 0, q, q, q, q, q, q, 0, 1.0,
                                                    q, q, None)
    assert tr(D=300) == _hip.DSP_ERR_ARGS
    assert tr(N=0) == _hip.DSP_ERR_ARGS
    assert tr(X=None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_mlp_predict(q, q, 5, 300, 3, arr, 10, q, None, None) == _hip.DSP_ERR_ARGS
    assert lib.dsp_mlp_predict(q, q, 0, 15, 3, arr, 10, q, None, None) == _hip.DSP_OK  # nothing to launch
    assert lib.dsp_mlp_dropout_mask(1, 0, 0, 0, 8, 0, q, None) == _hip.DSP_ERR_ARGS
