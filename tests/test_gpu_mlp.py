"""The fused MLP trainer (csrc/mlp.hip) on the MI355X against the restated reference
(tests/mlp_reference.py): dropout hash, training parity, state continuity, model independence,
predict, the two backends, and the Python surface.

Training parity measured on an MI355X, max |param - fp64| over the fp32 CPU reference's own max
deviation from fp64: 1.0 in seven of the eight cases, 5.3 in config_108 without dropout -- one
parameter with a near-zero gradient carries that maximum, see MARGIN in tests/mlp_reference.py and
DESIGN.md §4.5."""
import json

import numpy as np
import pytest
import torch

import mlp_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def gpu_train(D, hidden, C, batch, X, y, perm, w0, lrs, seeds, p, state=None, perm_stride=0):
    """One dsp_mlp_train launch (X [N, D] shared, or [K, N, D] with y [K, N]: a set per model); returns dict of numpy arrays (params, m, v [K, P], steps, loss_hist,
    acc_hist [K, E]).  state: the dict of an earlier launch to continue from."""
    from src.pipeline import mlp_train
    K = len(lrs)
    if state is None:
        params = _dev(np.tile(np.asarray(w0, dtype=np.float32), (K, 1)), torch.float32)
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        steps = torch.zeros(K, dtype=torch.int64, device=DEV)
    else:
        params, m, v = (_dev(state[k], torch.float32) for k in ('params', 'm', 'v'))
        steps = _dev(state['steps'], torch.int64)
    loss, acc = mlp_train(_dev(X, torch.float32), _dev(y, torch.int32), hidden, C, _dev(perm, torch.int32), params,
                          m, v, steps, _dev(np.asarray(lrs, dtype=np.float64), torch.float64),
                          _dev(np.asarray(seeds, dtype=np.uint32).view(np.int32), torch.int32), batch, dropout=p,
                          perm_stride=perm_stride)
    torch.cuda.synchronize()
    return dict(params=params.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy(), steps=steps.cpu().numpy(),
                loss_hist=loss.cpu().numpy(), acc_hist=acc.cpu().numpy())


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                              b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]) for k in a)


@pytest.mark.parametrize("width", [5, 33, 64])
@pytest.mark.parametrize("rows", [1, 34, 108])
def test_dropout_mask_equals_numpy_hash(rows, width):
    from src.pipeline import mlp_dropout_mask
    for step in (0, 7, (1 << 33) + 5):
        for layer in (0, 2):
            got = mlp_dropout_mask(R.PARITY_SEED, step, layer, rows, width, 0.3).cpu().numpy()
            assert np.array_equal(got.astype(bool), R.keep_mask(R.PARITY_SEED, step, layer, rows, width, 0.3))
    assert mlp_dropout_mask(3, 1, 0, rows, width, 0.0).cpu().numpy().all()


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("name", list(R.PARITY_SHAPES))
def test_training_parity(name, p):
    """Same initial weights, perm and masks: parameters, m, v within MARGIN (16) x (fp32 CPU reference's
    deviation from fp64) + FLOOR of the fp64 reference; histories likewise (loss: also 4 float32
    roundings of the value, it is stored as float32); every tensor also within the same formula over
    that tensor alone; the hit count of every epoch exact."""
    D, hidden, C, batch, N, X, y, perm, w0 = R.parity_inputs(name)
    ref = R.parity_reference(name, p, torch.float64)
    got = gpu_train(D, hidden, C, batch, X, y, perm, w0, [R.PARITY_LR], [R.PARITY_SEED], p)
    nb = -(-N // batch)
    assert got['steps'][0] == ref['steps'] == R.PARITY_EPOCHS * nb
    bound = R.parity_bound(name, p)
    raw = (bound - R.FLOOR) / R.MARGIN
    for key in ('params', 'm', 'v'):
        dev = float(np.max(np.abs(got[key][0].astype(np.float64) - ref[key])))
        print("%s p=%.1f %s: GPU deviation %.3g, fp32 CPU reference's %.3g, bound %.3g, ratio to bound %.3g"
              % (name, p, key, dev, raw, bound, dev / bound))
    for key in ('params', 'm', 'v'):
        dev = float(np.max(np.abs(got[key][0].astype(np.float64) - ref[key])))
        assert dev <= bound, (key, dev, bound)
    # tensor by tensor: an error in one tensor cannot hide under the maximum another one carries
    dims = R.layer_dims(D, hidden, C)
    ref32 = R.parity_reference(name, p, torch.float32)
    for key in ('params', 'm', 'v'):
        tdev = R.per_tensor_deviation(got[key][0], ref[key], dims)
        tbound = R.parity_bound_per_tensor(name, p, key)
        traw = R.per_tensor_deviation(ref32[key], ref[key], dims)
        for n, d, r, b in zip(R.tensor_names(dims), tdev, traw, tbound):
            print("%s p=%.1f %s %s: GPU deviation %.3g, fp32 CPU reference's %.3g, bound %.3g, ratio to bound %.3g"
                  % (name, p, key, n, d, r, b, d / b))
        assert (tdev <= tbound).all(), (key, tdev, tbound)
    lbound = R.parity_bound(name, p, 'loss_hist') + 4 * 2.0 ** -24 * float(np.max(ref['loss_hist']))
    ldev = float(np.max(np.abs(got['loss_hist'][0] - ref['loss_hist'])))
    print("%s p=%.1f loss_hist: GPU deviation %.3g, bound %.3g" % (name, p, ldev, lbound))
    assert ldev <= lbound
    # no train-mode logit row of these shapes is near a tie (tests/test_mlp_edges_host.py), so the hit
    # count of every epoch is the reference's
    for e in range(R.PARITY_EPOCHS):
        assert got['acc_hist'][0, e] == np.float32(int(ref['hits'][e]) / N), e
        assert round(float(got['acc_hist'][0, e]) * N) == int(ref['hits'][e]), e


def test_state_continuity():
    """4 epochs in one launch == 2 + 2 epochs in two launches, bit for bit, dropout on."""
    D, hidden, C, batch, N, X, y, perm, w0 = R.parity_inputs('config_108')
    rng = np.random.default_rng(3)
    perm4 = np.stack([rng.permutation(N) for _ in range(4)]).astype(np.int32)
    one = gpu_train(D, hidden, C, batch, X, y, perm4, w0, [1e-3], [9], 0.3)
    a = gpu_train(D, hidden, C, batch, X, y, perm4[:2], w0, [1e-3], [9], 0.3)
    b = gpu_train(D, hidden, C, batch, X, y, perm4[2:], w0, [1e-3], [9], 0.3, state=a)
    b['loss_hist'] = np.concatenate([a['loss_hist'], b['loss_hist']], axis=1)
    b['acc_hist'] = np.concatenate([a['acc_hist'], b['acc_hist']], axis=1)
    assert same_bits(one, b)
    assert not np.array_equal(a['params'], one['params'])


def test_model_independence_and_determinism():
    """Three models (different lr and seed) in one launch == three single-model launches; two
    identical launches are bitwise equal; a per-model perm stride selects each model's own order."""
    D, hidden, C, batch, N, X, y, perm, w0 = R.parity_inputs('odd_16')
    lrs, seeds = [1e-3, 3e-3, 1e-2], [1, 2, 0xFFFFFFF0]
    both = gpu_train(D, hidden, C, batch, X, y, perm, w0, lrs, seeds, 0.3)
    again = gpu_train(D, hidden, C, batch, X, y, perm, w0, lrs, seeds, 0.3)
    assert same_bits(both, again)
    for k in range(3):
        alone = gpu_train(D, hidden, C, batch, X, y, perm, w0, lrs[k:k + 1], seeds[k:k + 1], 0.3)
        assert same_bits(alone, {key: val[k:k + 1] for key, val in both.items()}), k
    assert not np.array_equal(both['params'][0], both['params'][1])
    rng = np.random.default_rng(4)
    perms = np.stack([np.stack([rng.permutation(N) for _ in range(2)]) for _ in range(3)]).astype(np.int32)
    strided = gpu_train(D, hidden, C, batch, X, y, perms, w0, lrs, seeds, 0.3, perm_stride=2 * N)
    for k in range(3):
        alone = gpu_train(D, hidden, C, batch, X, y, perms[k], w0, lrs[k:k + 1], seeds[k:k + 1], 0.3)
        assert same_bits(alone, {key: val[k:k + 1] for key, val in strided.items()}), k
    # a training set per model (x_stride / y_stride): the window comparison's launch
    Xs = np.stack([X, X[::-1] * 0.5, X + 1.0]).astype(np.float32)
    ys = np.stack([y, y[::-1], (y + 1) % C]).astype(np.int32)
    sets = gpu_train(D, hidden, C, batch, Xs, ys, perm, w0, lrs, seeds, 0.3)
    for k in range(3):
        alone = gpu_train(D, hidden, C, batch, Xs[k], ys[k], perm, w0, lrs[k:k + 1], seeds[k:k + 1], 0.3)
        assert same_bits(alone, {key: val[k:k + 1] for key, val in sets.items()}), k


@pytest.mark.parametrize("nq", [R.PREDICT_N, 1, 64, 65, 130])
def test_predict(nq):
    """Logits within PREDICT_MARGIN x (fp32 CPU forward's deviation) + FLOOR of the fp64 reference; labels equal
    on every row whose fp64 top-2 gap is not under twice that; Nq = 1 and Nq that are no multiple
    of the 64-row tile."""
    from src.pipeline import mlp_predict
    D, hidden, C, Xq, w = R.predict_inputs()
    l64, tol, excluded = R.predict_reference()
    pred, logits = mlp_predict(w, Xq[:nq], hidden, C, with_logits=True)
    pred, logits = pred.cpu().numpy(), logits.cpu().numpy()
    dev = float(np.max(np.abs(logits - l64[:nq])))
    print("predict nq=%d: logit deviation %.3g, tolerance %.3g" % (nq, dev, tol))
    assert dev <= tol
    keep = ~excluded[:nq]
    assert np.array_equal(pred[keep], l64[:nq].argmax(1)[keep])
    pred2, none = mlp_predict(w, Xq[:nq], hidden, C)
    assert none is None and np.array_equal(pred2.cpu().numpy(), pred)


def blobs(n=300, seed=0):
    rng = np.random.default_rng(seed)
    y = np.arange(n) % 3
    centers = np.array([[4.0, 0, 0, 0], [0, 4.0, 0, 0], [0, 0, 4.0, 0]])
    return (centers[y] + rng.normal(size=(n, 4))).astype(np.float32), y.astype(np.int64)


@pytest.mark.parametrize("backend", ["fused", "torch"])
def test_backends_learn_the_blobs(backend):
    """3 Gaussian blobs, 300 rows, 30 epochs, the same seed: train accuracy >= 0.95 and the last
    loss under the first (the CPU reference loop reaches 0.97+ here; the two backends are not
    bit-equal, torch's device dropout stream differs)."""
    from src.models import MLPTrainer
    X, y = blobs()
    t = MLPTrainer(4, [32, 16], 3, learning_rate=0.01, epochs=30, batch_size=16, seed=5, backend=backend)
    t.fit(X, y, verbose=False)
    assert len(t.train_losses) == 30 and len(t.train_accuracies) == 30
    assert t.train_losses[-1] < t.train_losses[0]
    assert t.train_accuracies[-1] >= 0.95, t.train_accuracies[-1]
    assert (t.predict(X) == y).mean() >= 0.95
    assert t._fused == (backend == "fused")


def test_surface_and_model_property(capsys):
    from src.models import create_classifier, fit_mlp_models
    X, y = blobs()
    clf = create_classifier('mlp', input_size=4, hidden_layers=[32, 16], num_classes=3, learning_rate=0.01,
                            epochs=20, batch_size=16, seed=2)
    clf.fit(X, y)
    out = capsys.readouterr().out
    assert "Epoch [10/20], Loss:" in out and "Epoch [20/20], Loss:" in out
    res = clf.evaluate(X, y)
    assert set(res) == {'accuracy', 'predictions', 'classification_report', 'confusion_matrix', 'train_losses',
                        'train_accuracies'}
    assert len(res['train_losses']) == 20 and res['accuracy'] >= 0.9
    net = clf.model  # nn.Sequential snapshot on the device
    with torch.no_grad():
        via_model = net(torch.as_tensor(X, device=DEV)).argmax(1).cpu().numpy()
    assert np.array_equal(via_model, clf.predict(X))
    # fit again continues (optimizer state and histories run on)
    clf.fit(X, y, verbose=False)
    assert len(clf.train_losses) == 40
    # the batched helper equals lone fused trainers bit for bit
    ts = fit_mlp_models(X, y, 4, [32, 16], 3, [0.01, 0.001], seeds=[2, 3], epochs=20, batch_size=16)
    lone = create_classifier('mlp', input_size=4, hidden_layers=[32, 16], num_classes=3, learning_rate=0.01,
                             epochs=20, batch_size=16, seed=2, backend='fused').fit(X, y, verbose=False)
    assert torch.equal(ts[0]._params, lone._params) and ts[0].train_losses == lone.train_losses
    assert ts[1].learning_rate == 0.001 and len(ts[1].train_losses) == 20
    # outside the fused plan 'auto' trains with the torch loop, 'fused' refuses
    wide = create_classifier('mlp', input_size=100, hidden_layers=[8], num_classes=3, epochs=1, seed=0)
    wide.fit(np.zeros((6, 100), np.float32), np.arange(6) % 3, verbose=False)
    assert wide._fused is False and len(wide.train_losses) == 1
    with pytest.raises(ValueError):
        create_classifier('mlp', input_size=100, hidden_layers=[8], num_classes=3, backend='fused').fit(
            np.zeros((6, 100), np.float32), np.arange(6) % 3, verbose=False)


@pytest.fixture()
def wav_dir(tmp_path):
    """3 classes x 5 synthetic clips (the 15-file pattern of tests/test_gpu_dataset.py)."""
    import wave
    from src.synth import make_clip
    for c in range(3):
        d = tmp_path / "data" / ("w%d" % c)
        d.mkdir(parents=True)
        for j in range(5):
            x = make_clip(2000 + 10 * c + j, n_samples=36000 + 1013 * j, label=c, n_classes=3)
            with wave.open(str(d / ("s%d.wav" % j)), "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(44100)
                w.writeframes(np.ascontiguousarray(x).tobytes())
    return str(tmp_path / "data")


def test_scripts_with_mlp(wav_dir, tmp_path, monkeypatch):
    import ablation_study
    import config
    import run
    import train_model
    # the learning-rate sweep: two rates in one launch, results.json + results_summary.txt
    out = ablation_study.ablation_learning_rate(wav_dir, [0.001, 0.01], save_dir=str(tmp_path / "lr"), verbose=False,
                                                epochs=5)
    assert sorted(out) == [0.001, 0.01]
    assert all(len(r['train_losses']) == 5 and 0.0 <= r['accuracy'] <= 1.0 for r in out.values())
    saved = json.load(open(tmp_path / "lr" / "results.json"))
    assert saved["experiment"] == "learning_rate" and set(saved["results"]) == {"0.001", "0.01"}
    text = open(tmp_path / "lr" / "results_summary.txt").read()
    assert "learning_rate" in text and "best accuracy" in text and "w0, w1, w2" in text
    # train_model fills config.MLP_* for 'mlp'
    monkeypatch.setattr(config, "MLP_EPOCHS", 20)
    X, y, classes, _ = train_model.load_dataset(wav_dir, verbose=False)
    r = train_model.train_and_evaluate(X, y, "mlp", test_size=0.4, verbose=False)
    clf = r["classifier"]
    assert (clf.hidden_layers, clf.batch_size, clf.learning_rate) == ([64, 64, 32], 108, 0.005)
    assert len(r["train_losses"]) == 20 and 0.0 <= r["train_accuracy"] <= 1.0
    # run.py --with-mlp: five rows; without the flag the four of before
    rd = tmp_path / "res"
    assert run.main(["--data-dir", wav_dir, "--results-dir", str(rd), "--experiment", "classifier",
                     "--with-mlp"]) == 0
    rows = json.load(open(rd / "exp1_classifier_comparison" / "results.json"))
    assert list(rows) == ["KNN", "Naive Bayes", "Decision Tree", "SVM", "MLP"]
    summary = open(rd / "exp1_classifier_comparison" / "results_summary.txt").read()
    assert "MLP:" in summary and "Precision:" in summary and "w2:" in summary
    assert run.main(["--data-dir", wav_dir, "--results-dir", str(tmp_path / "res4"), "--experiment",
                     "classifier"]) == 0
    assert list(json.load(open(tmp_path / "res4" / "exp1_classifier_comparison" / "results.json"))) == \
        ["KNN", "Naive Bayes", "Decision Tree", "SVM"]
    # the window comparison's three MLPs (one launch: the three splits have one shape)
    wres = run.last_experiment.experiment_window_comparison(with_mlp=True)
    assert all(set(r) == {"KNN", "SVM", "MLP"} and len(r["MLP"]["train_losses"]) == 20 for r in wres.values())
    assert "MLP:" in open(tmp_path / "res4" / "exp2_window_comparison" / "results_summary.txt").read()
