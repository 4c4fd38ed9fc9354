#!/usr/bin/env python3
"""Drop-in for the reference's compare_feature_methods.py (statistical 15-d vs padded E+ZCR
sequence features, then the same classifiers on both).

The reference walks the dataset twice, one file at a time, once per method (:43-64, :79-104),
and pads each sequence on the host (:106-115).  Here the dataset is decoded once into HBM
(src/dataset.PCMDataset) and ONE fused launch returns both the statistical matrix and the
per-frame sequences, already zero-padded to the longest sequence (PCMDataset.extract_both).
"""
import os
import sys

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import config  # noqa: E402
from src.dataset import PCMDataset  # noqa: E402
from src.feature_extraction import normalize_features  # noqa: E402
from src.models import create_classifier  # noqa: E402


# the reference's classifier table (compare_feature_methods.py:147-151)
CLASSIFIERS = {
    'KNN': ('knn', {'n_neighbors': 3}),
    'SVM': ('svm', {'C': 1.0, 'kernel': 'rbf'}),
    'Decision Tree': ('decision_tree', {}),
}


def load_both_methods(data_dir=None, frame_length=None, frame_shift=None, window_type='hamming', pitch=False, lpc=0):
    """:27-122 -> (X_statistical [n, 15], X_sequences_padded [n, max_len, 2], y, lengths); with
    ``pitch`` [n, 20] and [n, max_len, 3], the f0 statistics and the per-frame f0 appended
    (PCMDataset.extract_both); with ``lpc = n`` the n LPC cepstra per frame and their 2 n statistics behind
    those."""
    ds = PCMDataset(data_dir or config.DATA_DIR)
    X_stat, y, X_seq, lengths = ds.extract_both(frame_length or config.FRAME_LENGTH,
                                                frame_shift or config.FRAME_SHIFT, window_type,
                                                do_endpoint_detection=True, use_only_energy_zcr=True, pitch=pitch,
                                                sample_rate=config.SAMPLE_RATE, lpc=lpc)
    return X_stat, X_seq, y, lengths


def compare(data_dir=None, classifiers=None, test_size=0.2, random_state=42, dtw=False, dtw_template=False,
            hmm=False, pitch=False, lpc=0, vq=False, dhmm=False, dhmm_bw=False):
    """:124-214: each classifier on both feature sets, the reference's split and normalisation
    -> {classifier: {'statistical': acc, 'sequence': acc, 'diff': sequence - statistical}}.
    KNN on the flattened sequences (2 x max_frames columns) runs on the device like the 15-d
    case (dsp_knn_classify's chunked high-dimensional screen + fp64 re-rank).
    dtw=True (an extension) adds the row 'KNN-DTW': 'statistical' is the KNN's statistical accuracy,
    'sequence' the accuracy of k-NN under dynamic time warping (src.models.SequenceClassifier,
    n_neighbors=3) on the UNPADDED (E, ZCR) sequences of the same split.
    dtw_template=True (an extension) adds the row 'DTW-template' beside it: the same, for the nearest
    of one DBA template per class (src.models.TemplateClassifier, its defaults).
    hmm=True (an extension) adds the row 'HMM' beside them: the same, for one left-to-right Gaussian
    HMM per class (src.models.HmmClassifier, its defaults).
    vq=True (an extension) adds the row 'VQ' beside 'HMM': the same, for one vector-quantisation codebook
    per class (src.models.VqClassifier, its defaults).
    dhmm=True (an extension) adds the row 'VQ-HMM' after 'VQ': the same, for one discrete-observation HMM per
    class over one shared codebook (src.models.DiscreteHmmClassifier, its defaults).
    dhmm_bw=True (an extension) adds the row 'VQ-HMM (BW)' after it: the same classifier with Baum-Welch
    training and forward scoring (training='baum_welch', scoring='forward').
    pitch=True (an extension): every row runs on the 20-d matrix (the 15 columns plus five f0 statistics)
    and on the (E, ZCR, f0) sequences of the exact autocorrelation pitch track (src.pipeline.PitchTracker).
    lpc=n (an extension): the n LPC cepstra of every frame join the sequences and their means and standard
    deviations the matrix (src.pipeline.LpcAnalyzer).  The DTW, HMM and VQ kernels take at most 8 channels, so
    with one of their rows asked for, a sequence width 2 + pitch + n above 8 raises ValueError up front."""
    from sklearn.model_selection import train_test_split
    if isinstance(lpc, bool) or int(lpc) != lpc or not 0 <= lpc <= 64:
        raise ValueError("lpc is the number of cepstra per frame, 0 .. 64")
    if (dtw or dtw_template or hmm or vq or dhmm or dhmm_bw) and 2 + bool(pitch) + lpc > 8:
        raise ValueError("the DTW and HMM rows take sequences of at most 8 channels: E, ZCR%s and %d cepstra are %d"
                         % (", f0" if pitch else "", lpc, 2 + bool(pitch) + lpc))
    X_stat, X_seq, y, lengths = load_both_methods(data_dir, pitch=pitch, lpc=lpc)
    X_flat = X_seq.reshape(len(X_seq), -1)
    Xs_tr, Xs_te, y_tr, y_te = train_test_split(X_stat, y, test_size=test_size, random_state=random_state,
                                                stratify=y)
    Xq_tr, Xq_te, _, _ = train_test_split(X_flat, y, test_size=test_size, random_state=random_state, stratify=y)
    Xs_tr, m, sd = normalize_features(Xs_tr)
    Xs_te, _, _ = normalize_features(Xs_te, m, sd)
    Xq_tr, m, sd = normalize_features(Xq_tr)
    Xq_te, _, _ = normalize_features(Xq_te, m, sd)
    results = {}
    for name, (kind, params) in (classifiers or CLASSIFIERS).items():
        acc = {}
        for method, (tr, te) in (("statistical", (Xs_tr, Xs_te)), ("sequence", (Xq_tr, Xq_te))):
            clf = create_classifier(kind, **params)
            clf.fit(tr, y_tr)
            acc[method] = float(clf.evaluate(te, y_te)['accuracy'])
        results[name] = {'statistical': acc['statistical'], 'sequence': acc['sequence'],
                         'diff': acc['sequence'] - acc['statistical']}
    if dtw or dtw_template or hmm or vq or dhmm or dhmm_bw:
        tr, te = train_test_split(np.arange(len(y)), test_size=test_size, random_state=random_state, stratify=y)
        lengths = np.asarray(lengths)
        if 'KNN' in results:
            stat_acc = results['KNN']['statistical']
        else:
            kind, params = CLASSIFIERS['KNN']
            knn = create_classifier(kind, **params).fit(Xs_tr, y_tr)
            stat_acc = float(knn.evaluate(Xs_te, y_te)['accuracy'])
        rows = ([('KNN-DTW', 'dtw_knn', {'n_neighbors': 3})] if dtw else []) + \
               ([('DTW-template', 'dtw_template', {})] if dtw_template else []) + \
               ([('HMM', 'hmm', {})] if hmm else []) + \
               ([('VQ', 'vq', {})] if vq else []) + \
               ([('VQ-HMM', 'dhmm', {})] if dhmm else []) + \
               ([('VQ-HMM (BW)', 'dhmm', {'training': 'baum_welch', 'scoring': 'forward'})] if dhmm_bw else [])
        for name, kind, params in rows:
            clf = create_classifier(kind, **params).fit(X_seq[tr], y[tr], lengths=lengths[tr])
            seq_acc = float(clf.evaluate(X_seq[te], y[te], lengths=lengths[te])['accuracy'])
            results[name] = {'statistical': stat_acc, 'sequence': seq_acc, 'diff': seq_acc - stat_acc}
    return results


if __name__ == "__main__":
    res = compare()
    for name, r in res.items():
        print("%-15s statistical %.4f  sequence %.4f  diff %+.4f" % (name, r['statistical'], r['sequence'], r['diff']))
    print("mean  statistical %.4f  sequence %.4f" % (np.mean([r['statistical'] for r in res.values()]),
                                                      np.mean([r['sequence'] for r in res.values()])))
