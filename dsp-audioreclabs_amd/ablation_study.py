#!/usr/bin/env python3
"""Drop-in for the reference's ablation_study.py (learning-rate / frame-length / frame-shift sweeps)
on MI355X.

The reference reloads and re-processes every WAV file for each setting
(ablation_study.py:146-163, 230-247 via train_model.load_dataset).  Here the dataset is decoded
once into HBM and each setting is one fused kernel launch over all clips (train_model.py,
src/dataset.py).  The learning-rate sweep (:27-109) trains all its MLPs in one launch of the
fused trainer, a workgroup per rate (src/models.fit_mlp_models).  Results are written as JSON with
the reference's text summary (:363-410) beside it (its plots need matplotlib/seaborn and are out
of scope).  The default classifier stays the device KNN (the reference's is 'mlp'; --classifier mlp
selects it), and 'all' runs the two frame sweeps as before; --experiment lr runs the rate sweep.

    python ablation_study.py --data-dir <dir> --experiment lr|frame_length|frame_shift|all
"""
import argparse
import json
import os
import sys
from datetime import datetime

PKG = os.path.dirname(os.path.abspath(__file__))
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import config  # noqa: E402
from train_model import load_dataset, train_and_evaluate  # noqa: E402

FRAME_LENGTH_MS_RANGE = [8, 10, 12, 15, 18, 20, 25, 30, 35, 40, 45, 50]  # config.py:81
FRAME_SHIFT_MS_RANGE = [3, 5, 7, 8, 10, 12, 15, 18, 20, 25, 30]  # config.py:85


def _save_ablation_results(results, save_dir, name, data_dir, classifier_type, class_names):
    """results.json, and results_summary.txt with the fields of the reference's summary (:363-410):
    experiment, dataset, classes, parameter, time, train / test accuracy per value, the best value."""
    os.makedirs(save_dir, exist_ok=True)
    dataset = os.path.basename(os.path.abspath(data_dir))
    with open(os.path.join(save_dir, 'results.json'), 'w') as f:
        json.dump({'experiment': name, 'dataset': dataset, 'classifier': classifier_type,
                   'results': {str(k): v for k, v in results.items()}}, f, indent=1)
    best = max(results, key=lambda k: results[k]['accuracy'])
    lines = ["=" * 70, "ablation: %s (%s)" % (name, classifier_type), "=" * 70, "",
             "dataset: %s" % dataset, "classes: %s" % ", ".join(class_names), "parameter: %s" % name,
             "time: %s" % datetime.now().strftime('%Y-%m-%d %H:%M:%S'), "",
             "%-15s %-15s %-15s" % ("value", "train accuracy", "test accuracy"), "-" * 70]
    lines += ["%-15s %-15.4f %-15.4f" % (k, r['train_accuracy'], r['accuracy']) for k, r in results.items()]
    lines += ["", "=" * 70, "best value: %s" % best, "best accuracy: %.4f" % results[best]['accuracy'], "=" * 70]
    with open(os.path.join(save_dir, 'results_summary.txt'), 'w', encoding='utf-8') as f:
        f.write("\n".join(lines) + "\n")


def _sweep(data_dir, name, values, kw_of, classifier_type, save_dir, verbose):
    results = {}
    for v in values:
        X, y, class_names, _ = load_dataset(data_dir, window_type='hamming', verbose=verbose, **kw_of(v))
        r = train_and_evaluate(X, y, classifier_type=classifier_type, verbose=verbose)
        results[v] = {'accuracy': float(r['accuracy']), 'train_accuracy': float(r['train_accuracy']),
                      'confusion_matrix': r['confusion_matrix'].tolist()}
    if save_dir:
        _save_ablation_results(results, save_dir, name, data_dir, classifier_type, class_names)
    return results


def ablation_learning_rate(data_dir=None, learning_rates=None, classifier_type='mlp', save_dir=None,
                           verbose=True, **mlp_params):
    """ablation_study.py:27-109: test / train accuracy per MLP learning rate, features at config's
    frame sizes.  Every rate is one model of a single fused launch per epoch chunk (model k seeded
    with k); ``mlp_params`` (hidden_layers, epochs, batch_size) override config.MLP_*."""
    import numpy as np
    from sklearn.metrics import accuracy_score
    from sklearn.model_selection import train_test_split
    from src.feature_extraction import normalize_features
    from src.models import fit_mlp_models
    if classifier_type != 'mlp':
        raise ValueError("the learning-rate sweep concerns the MLP only")
    data_dir = data_dir or config.DATA_DIR
    save_dir = save_dir if save_dir is not None else os.path.join(config.RESULTS_DIR, 'ablation_learning_rate')
    learning_rates = list(learning_rates or config.LEARNING_RATES)
    X, y, class_names, _ = load_dataset(data_dir, window_type='hamming', verbose=verbose)
    X_tr, X_te, y_tr, y_te = train_test_split(X, y, test_size=0.2, random_state=42, stratify=y)
    X_tr, mean, std = normalize_features(X_tr)
    X_te, _, _ = normalize_features(X_te, mean, std)
    trainers = fit_mlp_models(X_tr, y_tr, X_tr.shape[1], mlp_params.get('hidden_layers', config.MLP_HIDDEN_LAYERS),
                              len(np.unique(y)), learning_rates, epochs=mlp_params.get('epochs', config.MLP_EPOCHS),
                              batch_size=mlp_params.get('batch_size', config.MLP_BATCH_SIZE))
    results = {}
    for lr, t in zip(learning_rates, trainers):
        r = t.evaluate(X_te, y_te)
        results[lr] = {'accuracy': float(r['accuracy']),
                       'train_accuracy': float(accuracy_score(y_tr, t.predict(X_tr))),
                       'confusion_matrix': r['confusion_matrix'].tolist(),
                       'train_losses': [float(v) for v in t.train_losses],
                       'train_accuracies': [float(v) for v in t.train_accuracies]}
        if verbose:
            print("lr %g: test accuracy %.4f, train accuracy %.4f" % (lr, results[lr]['accuracy'],
                                                                      results[lr]['train_accuracy']))
    if save_dir:
        _save_ablation_results(results, save_dir, 'learning_rate', data_dir, classifier_type, class_names)
    return results


def ablation_frame_length(data_dir=None, frame_lengths_ms=None, classifier_type='knn', save_dir=None,
                          verbose=True):
    """ablation_study.py:112-193: accuracy per frame length (ms), frame shift from config."""
    data_dir = data_dir or config.DATA_DIR
    save_dir = save_dir if save_dir is not None else os.path.join(config.RESULTS_DIR, 'ablation_frame_length')
    return _sweep(data_dir, 'frame_length_ms', frame_lengths_ms or FRAME_LENGTH_MS_RANGE,
                  lambda v: {'frame_length_ms': v}, classifier_type, save_dir, verbose)


def ablation_frame_shift(data_dir=None, frame_shifts_ms=None, classifier_type='knn', save_dir=None,
                         verbose=True):
    """ablation_study.py:196-277: accuracy per frame shift (ms), frame length from config."""
    data_dir = data_dir or config.DATA_DIR
    save_dir = save_dir if save_dir is not None else os.path.join(config.RESULTS_DIR, 'ablation_frame_shift')
    return _sweep(data_dir, 'frame_shift_ms', frame_shifts_ms or FRAME_SHIFT_MS_RANGE,
                  lambda v: {'frame_shift_ms': v}, classifier_type, save_dir, verbose)


def main(argv=None):
    ap = argparse.ArgumentParser(description="learning rate / frame length / shift ablations (MI355X)")
    ap.add_argument('--data-dir', type=str, default=None)
    ap.add_argument('--experiment', default='all', choices=['all', 'lr', 'frame_length', 'frame_shift'])
    ap.add_argument('--classifier', default='knn', choices=['knn', 'svm', 'naive_bayes', 'decision_tree', 'mlp'])
    ap.add_argument('--results-dir', type=str, default=None)
    a = ap.parse_args(argv)
    data_dir = os.path.abspath(os.path.expanduser(a.data_dir)) if a.data_dir else config.DATA_DIR
    if not os.path.isdir(data_dir):
        print("data directory not found: %s (use --data-dir)" % data_dir)
        return 1
    rd = a.results_dir or config.RESULTS_DIR
    out = {}
    if a.experiment == 'lr':
        out['learning_rate'] = ablation_learning_rate(data_dir, save_dir=os.path.join(rd, 'ablation_learning_rate'))
    if a.experiment in ('all', 'frame_length'):
        out['frame_length'] = ablation_frame_length(data_dir, classifier_type=a.classifier,
                                                    save_dir=os.path.join(rd, 'ablation_frame_length'))
    if a.experiment in ('all', 'frame_shift'):
        out['frame_shift'] = ablation_frame_shift(data_dir, classifier_type=a.classifier,
                                                  save_dir=os.path.join(rd, 'ablation_frame_shift'))
    print({k: {kk: vv['accuracy'] for kk, vv in v.items()} for k, v in out.items()})
    return 0


if __name__ == '__main__':
    sys.exit(main())
