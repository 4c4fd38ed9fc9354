"""Drop-in for the reference's src/models.py (classifiers) on MI355X.

``TraditionalClassifier('knn')`` (models.py:18-72) -- the classifier on the north-star path --
runs the exact k-NN kernel (csrc/knn.hip, dsp_knn_classify): the same neighbours, distances and
majority vote as scikit-learn's KNeighborsClassifier(n_neighbors=k) (kd_tree, Euclidean,
uniform weights, scipy.stats.mode: smallest label on ties).

``TraditionalClassifier('svm')`` trains with scikit-learn's SVC (libsvm) exactly as the reference
does -- a device SMO would converge to another dual solution -- and predicts the
fitted RBF model on the device (csrc/svm.hip, dsp_svc_predict): libsvm's kernel
sums and one-vs-one vote in fp64, each row certified against a derived rounding bound.

``TraditionalClassifier('naive_bayes')`` keeps a complete scikit-learn ``GaussianNB`` in ``.model``
and predicts it on the device (csrc/gnb.hip, dsp_gnb_predict): the joint log
likelihood in fp64, each row's argmax certified against a derived rounding bound.  ``fit`` on a
float64 device tensor runs dsp_gnb_fit -- numpy's own sequential sums, so theta_, var_, epsilon_ and
class_prior_ are GaussianNB.fit's bits -- and with host rows it is scikit-learn's fit.

``TraditionalClassifier('decision_tree')`` trains with scikit-learn (the best-split search draws
its feature order from scikit-learn's RNG and breaks ties by visiting order) and
walks the fitted tree on the device (csrc/tree.hip, dsp_tree_predict): comparisons only, so
``predict`` and ``apply`` are scikit-learn's with no tolerance.

These three share one path (``TraditionalClassifier._certified``): the fitted model is uploaded once
(``pipeline.SvcIndex`` / ``GnbIndex`` / ``TreeIndex``) and again when the model is refitted, host rows
or float64 device rows are queried, and the rows the device did not settle -- near ties the bound
cannot decide, for the tree a NaN or a value that is not finite as float32 -- are answered by the
model's own method on those rows alone, so the labels are scikit-learn's.  A model or rows outside
the kernel's plan (``Index.in_plan``: another SVC kernel, sparse input, more than 64 classes, a
multi-output tree) go to scikit-learn entirely; ``last_predict_stats`` says which path ran.

``SequenceClassifier`` / ``create_classifier('dtw_knn')`` (an extension: the reference has no
sequence classifier) is k-NN under dynamic time warping on the per-frame sequences (csrc/dtw.hip,
dsp_dtw_knn): an exact fp64 distance, the KNN's voting and tie rules.
``TemplateClassifier`` / ``create_classifier('dtw_template')`` keeps one DBA template per class instead
of the training set (csrc/dtw_align.hip, dsp_dtw_dba_update).
``HmmClassifier`` / ``create_classifier('hmm')`` keeps one left-to-right Gaussian HMM per class, trained
by Viterbi re-estimation (csrc/hmm.hip, dsp_hmm_score / dsp_hmm_align / dsp_hmm_accumulate, DESIGN.md
§4.10): scores, state paths and re-estimated models defined bit for bit.
``VqClassifier`` / ``create_classifier('vq')`` keeps one vector-quantisation codebook per class, trained by
LBG binary splitting (csrc/vq.hip, dsp_vq_score / dsp_vq_assign / dsp_vq_accumulate):
nearest codewords, distortions and re-estimated codebooks defined bit for bit.

``MLPTrainer`` (models.py:109-221) trains the reference's MLP with the fused on-device trainer
(csrc/mlp.hip: dsp_mlp_train / dsp_mlp_predict) -- the whole serial SGD loop of
models.py:146-194 in one persistent workgroup, many epochs per launch -- or, outside that kernel's
plan, with the reference's own loop in plain torch on the device.  ``fit_mlp_models`` trains a
learning-rate sweep in one launch.
"""
import numpy as np

from .pipeline import GnbIndex, KnnIndex, SvcIndex, TreeIndex, _as_host, gaussian_nb_fit


def _is_device_f64(X):
    import torch
    return isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float64


# the scikit-learn-backed types: the uploaded form of the fitted model and, from a query's outputs, the
# rows the device did not settle (near ties of the certificate; for the tree a NaN or a value that is
# not finite as float32)
_DEVICE = {'svm': (SvcIndex, lambda pred, dec, certified: certified == 0),
           'naive_bayes': (GnbIndex, lambda pred, jll, certified: certified == 0),
           'decision_tree': (TreeIndex, lambda pred, leaf: pred < 0)}


class TraditionalClassifier:
    """models.py:18-72: fit / predict / evaluate with the reference's hyper-parameters."""

    def __init__(self, classifier_type='knn', **kwargs):
        self.classifier_type = classifier_type
        self._index = None  # the device's copy of the fitted model (knn: of the training set)
        if classifier_type == 'knn':
            self.n_neighbors = int(kwargs.get('n_neighbors', 3))
            self.model = None
            return
        if classifier_type == 'naive_bayes':
            from sklearn.naive_bayes import GaussianNB
            self.model = GaussianNB()
        elif classifier_type == 'decision_tree':
            from sklearn.tree import DecisionTreeClassifier
            self.model = DecisionTreeClassifier(max_depth=kwargs.get('max_depth', None), random_state=42)
        elif classifier_type == 'svm':
            from sklearn.svm import SVC
            self.model = SVC(C=kwargs.get('C', 1.0), kernel=kwargs.get('kernel', 'rbf'), random_state=42)
        else:
            raise ValueError(f"不支持的分类器类型: {classifier_type}")
        # which path the last predict / apply / decision_function took (device: the kernel ran;
        # uncertified: rows of it that the device did not settle)
        self.last_predict_stats = {'device': False, 'uncertified': 0}

    def fit(self, X_train, y_train):
        if self.classifier_type != 'knn':
            self._index = None  # the fitted model is uploaded at the first predict
            if self.classifier_type == 'naive_bayes' and _is_device_f64(X_train):
                return self._fit_nb_device(X_train, y_train)
            self.model.fit(X_train, y_train)
            return self
        X = np.asarray(X_train, dtype=np.float64)
        y = np.asarray(y_train)
        if len(X) < self.n_neighbors:
            raise ValueError("Expected n_neighbors <= n_samples_fit, but n_neighbors = %d, n_samples_fit = %d"
                             % (self.n_neighbors, len(X)))
        # classes_ sorted as in scikit-learn; the vote's smallest-index tie break is then the
        # smallest label (scipy.stats.mode)
        self.classes_, codes = np.unique(y, return_inverse=True)
        # the reference set on the device, converted for the screen at the first query and kept
        self._index = KnnIndex(X, codes.astype(np.int32), self.n_neighbors, n_classes=len(self.classes_))
        return self

    def kneighbors(self, X_test):
        """(distances, indices) [n, k] like KNeighborsClassifier.kneighbors(X_test)."""
        idx, dist, _ = self._index.query(np.asarray(X_test, dtype=np.float64))
        return dist.cpu().numpy(), idx.cpu().numpy().astype(np.int64)

    def _fit_nb_device(self, X, y):
        """GaussianNB.fit of device rows with dsp_gnb_fit; .model ends up a complete GaussianNB."""
        m = self.model
        y = _as_host(y)
        classes, codes = np.unique(y, return_inverse=True)
        if X.dim() != 2 or X.shape[1] < 2 or len(classes) > 64 or m.priors is not None or len(y) != X.shape[0]:
            m.fit(X.cpu().numpy(), y)  # outside dsp_gnb_fit's plan (one column: numpy sums pairwise)
            return self
        theta, var, count, eps = gaussian_nb_fit(X, codes.astype(np.int32), len(classes), m.var_smoothing)
        m.classes_, m.n_features_in_ = classes, int(X.shape[1])
        m.epsilon_ = np.float64(eps.item())
        m.theta_, m.var_ = theta.cpu().numpy(), var.cpu().numpy()
        m.class_count_ = count.cpu().numpy().astype(np.float64)
        m.class_prior_ = m.class_count_ / m.class_count_.sum()
        return self

    # -- SVC, Naive Bayes and Decision Tree on the device (models.py:37-47, :52-58) -------------
    def _certified(self, X, method, answer, redo=None, **outputs):
        """``method`` (the model's predict, apply or _decision_function) of X, computed on the device:
        ``answer`` of the query's outputs as numpy arrays, and ``method``'s own result for the rows the
        device did not settle, or for the rows ``redo`` of the outputs marks.  A model or rows outside
        the kernel's plan are ``method``'s entirely."""
        Index, unsettled = _DEVICE[self.classifier_type]
        m = self.model
        if not Index.in_plan(m, X):
            self.last_predict_stats = {'device': False, 'uncertified': 0}
            return method(X)
        # uploaded once per fitted model (a refit, also one made on self.model directly, replaces
        # support_vectors_ / theta_ / tree_)
        if self._index is None or self._index.source is not Index.source_of(m):
            self._index = Index(m)
        if not hasattr(X, 'cpu'):  # device rows stay where they are
            X = np.asarray(X, dtype=np.float64)
        out = [None if t is None else t.cpu().numpy() for t in self._index.query(X, **outputs)]
        rows = np.flatnonzero(unsettled(*out))
        self.last_predict_stats = {'device': True, 'uncertified': len(rows)}  # (before method may raise)
        y = answer(*out)
        if redo is not None:
            rows = np.flatnonzero(redo(*out))
        if len(rows):
            y[rows] = method(_as_host(X[rows]))
        return y

    def decision_function(self, X):
        """SVC.decision_function with decision_function_shape='ovo' ([n, C(C-1)/2]; [n] and
        scikit-learn's flipped sign for two classes).  SVM only."""
        if self.classifier_type != 'svm':
            raise AttributeError("decision_function is the SVM's")
        # dec is within its derived bound on every row, certified or not, so a near tie is not redone.
        # A row with a NaN or an inf comes back as NaN in every dec_p (csrc/svm.hip): the model is
        # asked for the rows whose dec is not finite, and raises for them as SVC.decision_function does.
        return self._certified(X, self.model._decision_function, with_dec=True,
                               redo=lambda pred, dec, certified: ~np.isfinite(dec).all(axis=1),
                               answer=lambda pred, dec, certified: -dec.ravel() if dec.shape[1] == 1 else dec)

    def apply(self, X):
        """DecisionTreeClassifier.apply: the leaf's node index per row, int64.  Decision tree only."""
        if self.classifier_type != 'decision_tree':
            raise AttributeError("apply is the decision tree's")
        return self._certified(X, self.model.apply, lambda pred, leaf: leaf.astype(np.int64))

    def predict(self, X_test):
        if self.classifier_type == 'knn':
            _, _, pred = self._index.query(np.asarray(X_test, dtype=np.float64))
            return self.classes_[pred.cpu().numpy()]
        outputs = {'with_leaf': False} if self.classifier_type == 'decision_tree' else {}
        return self._certified(X_test, self.model.predict, lambda pred, *_: self.model.classes_[np.maximum(pred, 0)],
                               **outputs)

    def evaluate(self, X_test, y_test):
        from sklearn.metrics import accuracy_score, classification_report, confusion_matrix
        y_pred = self.predict(X_test)
        return {
            'accuracy': accuracy_score(y_test, y_pred),
            'predictions': y_pred,
            'classification_report': classification_report(y_test, y_pred, output_dict=True, zero_division=0),
            'confusion_matrix': confusion_matrix(y_test, y_pred),
        }


# ==================== DTW nearest neighbours on the frame sequences ====================

def _as_padded(X, lengths):
    """(padded float64 [N, T, F], lengths int32 [N]) from a list of [n_i, F] arrays, or from a
    padded [N, T, F] array with its lengths.  Non-finite valid frames raise ValueError."""
    if isinstance(X, (list, tuple)):
        if lengths is not None:
            raise ValueError("a list of sequences carries its own lengths")
        seqs = [np.asarray(x, dtype=np.float64) for x in X]
        seqs = [x.reshape(-1, 1) if x.ndim == 1 else x for x in seqs]
        if not seqs or any(x.ndim != 2 or x.shape[1] != seqs[0].shape[1] for x in seqs):
            raise ValueError("X must be a non-empty list of [n_i, F] arrays with one F")
        n = np.array([len(x) for x in seqs], dtype=np.int32)
        if n.min() < 1:
            raise ValueError("empty sequence at index %d" % int(np.argmin(n)))
        out = np.zeros((len(seqs), int(n.max()), seqs[0].shape[1]))
        for i, x in enumerate(seqs):
            out[i, :len(x)] = x
    else:
        out = np.array(_as_host(X), dtype=np.float64)  # a copy: the padding is rewritten below
        if out.ndim != 3:
            raise ValueError("X must be a list of [n_i, F] arrays or a padded [N, T, F] array")
        if lengths is None:
            raise ValueError("a padded [N, T, F] array needs lengths: trailing zero rows could be real frames")
        n = _as_host(lengths).astype(np.int32).reshape(-1)
        if len(n) != len(out) or (len(n) and (n.min() < 1 or n.max() > out.shape[1])):
            raise ValueError("lengths must be one per sequence, in [1, %d]" % out.shape[1])
    valid = np.arange(out.shape[1])[None, :] < n[:, None]
    if not np.isfinite(out[valid]).all():
        raise ValueError("Input sequences contain NaN or infinity")
    out[~valid] = 0.0  # the padding is never read as a frame; keep it finite
    return out, n


class SequenceClassifier:
    """k nearest neighbours under dynamic time warping on the per-frame sequences -- the textbook
    classifier for the (E, M, ZCR) frame features (an extension: the reference only flattens the
    zero-padded sequences, compare_feature_methods.py:106-115).  csrc/dtw.hip (dsp_dtw_knn,
    DESIGN.md §4.8): the exact fp64 DTW of include/dsp_audiorec.h, KNeighborsClassifier's voting and
    tie rules as in ``TraditionalClassifier('knn')``.

    X is a list of [n_i, F] arrays, or a padded [N, T, F] array together with ``lengths``.
    window     None: unconstrained; else the Sakoe-Chiba band's half width in frames.
    normalize  each feature channel's mean and population standard deviation over all valid frames
               of the training sequences (numpy, std == 0 -> 1, as normalize_features), applied to
               training and query sequences -- raw energies would drown the ZCR in the local cost.
    No CPU path: ``predict`` raises HipError without a HIP device (``fit`` and constructing need none).
    """

    def __init__(self, n_neighbors=3, window=None, normalize=True):
        self.n_neighbors, self.window, self.normalize = int(n_neighbors), window, bool(normalize)
        self._index = None

    def _scale(self, X, n):
        if not self.normalize:
            return X
        valid = np.arange(X.shape[1])[None, :] < n[:, None]
        out = (X - self.mean_) / self.std_
        out[~valid] = 0.0
        return out

    def _training_set(self, X, y, lengths):
        """(scaled padded X, lengths, class codes) of a training set; sets mean_, std_ and classes_."""
        X, n = _as_padded(X, lengths)
        y = np.asarray(y)
        if len(y) != len(X):
            raise ValueError("%d labels for %d sequences" % (len(y), len(X)))
        if len(X) < self.n_neighbors:
            raise ValueError("Expected n_neighbors <= n_samples_fit, but n_neighbors = %d, n_samples_fit = %d"
                             % (self.n_neighbors, len(X)))
        if self.normalize:
            frames = X[np.arange(X.shape[1])[None, :] < n[:, None]]  # all valid frames, [sum n_i, F]
            self.mean_ = np.mean(frames, axis=0)
            std = np.std(frames, axis=0)
            self.std_ = np.where(std == 0, 1.0, std)
        # classes_ sorted as in scikit-learn: the vote's smallest-index tie break is the smallest label
        self.classes_, codes = np.unique(y, return_inverse=True)
        return self._scale(X, n), n, codes.astype(np.int32)

    def fit(self, X, y, lengths=None):
        self._fit_X, self._fit_n, self._codes = self._training_set(X, y, lengths)
        self._index = None  # uploaded at the first query
        return self

    def _query(self, X, lengths):
        from .pipeline import DtwIndex
        Xq, nq = _as_padded(X, lengths)
        if Xq.shape[2] != self._fit_X.shape[2]:
            raise ValueError("X has %d feature channels, the fitted sequences %d" % (Xq.shape[2], self._fit_X.shape[2]))
        if self._index is None:
            self._index = DtwIndex(self._fit_X, self._fit_n, self._codes, self.n_neighbors,
                                   n_classes=len(self.classes_), window=self.window, check_finite=False)
        return self._index.query(self._scale(Xq, nq), nq, check_finite=False)

    def kneighbors(self, X, lengths=None):
        """(distances float64, indices int64) [n, k], ascending DTW distance."""
        idx, dist, _ = self._query(X, lengths)
        return dist.cpu().numpy(), idx.cpu().numpy().astype(np.int64)

    def predict(self, X, lengths=None):
        _, _, pred = self._query(X, lengths)
        return self.classes_[pred.cpu().numpy()]

    def evaluate(self, X, y, lengths=None):
        from sklearn.metrics import accuracy_score, classification_report, confusion_matrix
        y_pred = self.predict(X, lengths)
        return {
            'accuracy': accuracy_score(y, y_pred),
            'predictions': y_pred,
            'classification_report': classification_report(y, y_pred, output_dict=True, zero_division=0),
            'confusion_matrix': confusion_matrix(y, y_pred),
        }


def medoid_index(cost_rows):
    """The medoid rule on the candidates' squared-distance rows d * d [n_candidates, M]: the cost of
    a candidate is the sequential sum over the members in order (cumsum), the smallest wins, ties go
    to the earliest candidate."""
    return int(np.argmin(np.cumsum(cost_rows, axis=1)[:, -1]))


class TemplateClassifier(SequenceClassifier):
    """Template matching, the classical form of the isolated-word recogniser: one reference pattern
    per class, the class's DTW barycentre (DBA; Petitjean, Ketterlin, Gancarski 2011), and the label of
    the nearest template under DTW.  csrc/dtw_align.hip (dsp_dtw_dba_update).  Input
    handling and normalisation are ``SequenceClassifier``'s; prediction is its 1-NN over the templates
    (``n_classes`` dynamic programmes per query instead of one per training sequence).

    n_iter             DBA updates, all classes in each call.
    medoid_candidates  each class starts from its medoid among the first ``medoid_candidates`` members
                       (training order): the candidate with the smallest sum of squared DTW distances
                       to all members of the class (``medoid_index``).
    After ``fit``: templates_ float64 [C, T, F] (normalised units, zeros behind each length),
    template_lengths_ int32 [C], inertia_ float64 [n_iter, C] (row t: each class's sum of squared DTW
    distances to the template that update t started from).
    No CPU path: ``fit`` and ``predict`` raise HipError without a HIP device (constructing needs none).
    """

    def __init__(self, n_iter=10, window=None, normalize=True, medoid_candidates=256):
        super().__init__(n_neighbors=1, window=window, normalize=normalize)
        self.n_iter, self.medoid_candidates = int(n_iter), int(medoid_candidates)
        if self.n_iter < 0 or self.medoid_candidates < 1:
            raise ValueError("n_iter must be >= 0 and medoid_candidates >= 1")

    def fit(self, X, y, lengths=None):
        from .pipeline import DbaUpdater, dtw_pairwise
        X, n, codes = self._training_set(X, y, lengths)
        C = len(self.classes_)
        order = np.argsort(codes, kind="stable")  # each class's members in training order
        start = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=C))])
        medoids = []
        for c in range(C):
            mem = order[start[c]:start[c + 1]]
            cand = mem[:self.medoid_candidates]
            d = dtw_pairwise(X[cand], n[cand], X[mem], n[mem], window=self.window, check_finite=False).cpu().numpy()
            medoids.append(cand[medoid_index(d * d)])
        tmpl, len_t = X[medoids], n[medoids]
        updater = DbaUpdater(X, n, start, order, window=self.window, check_finite=False)
        inertia = np.zeros((self.n_iter, C))
        for t in range(self.n_iter):
            tmpl, inert = updater.update(tmpl, len_t)
            inertia[t] = inert.cpu().numpy()
        self.templates_ = _as_host(tmpl)
        self.template_lengths_, self.inertia_ = len_t.astype(np.int32), inertia
        self._fit_X, self._fit_n, self._codes = self.templates_, self.template_lengths_, np.arange(C, dtype=np.int32)
        self._index = None  # uploaded at the first query
        return self


class HmmClassifier(SequenceClassifier):
    """One left-to-right Gaussian hidden Markov model per class, trained by Viterbi re-estimation
    (segmental k-means), and the label of the model with the best state path -- the textbook step
    after DTW templates: a mean and a variance per state, and a cost for staying in a state, which
    models duration.  csrc/hmm.hip (dsp_hmm_score, dsp_hmm_align, dsp_hmm_accumulate).
    Input handling and normalisation are ``SequenceClassifier``'s.

    n_states     states per model: an int, or one value per class (in the order of the sorted class
                 values), each in 1 .. 32.
    n_iter       rounds of align -> accumulate -> rebuild after the uniform start; training stops
                 early when a round changes no segment boundary.
    var_floor    lower bound of every variance (normalised units).
    trans_floor  p_stay is clamped to [trans_floor, 1 - trans_floor].
    A training sequence shorter than its class's n_states is left out of that class's statistics; a
    class none of whose members is long enough raises ValueError at ``fit``.  ``predict`` raises
    ValueError for a query with fewer frames than every model has states (``score_samples`` returns
    its row of +inf).
    After ``fit``: model_ (``pipeline.HmmModelSet``: mean, var, w, g, stay, adv, n_states), totals_
    float64 [rounds run, C] (row t: each class's sum of its members' scores under the model round t
    started from), n_iter_ the rounds run.
    No CPU path: ``fit`` and ``predict`` raise HipError without a HIP device (constructing needs none).
    """

    def __init__(self, n_states=5, n_iter=10, var_floor=1e-3, trans_floor=1e-3, normalize=True):
        super().__init__(n_neighbors=1, window=None, normalize=normalize)
        from .pipeline import HMM_MAX_STATES
        states = np.asarray(n_states)
        if states.ndim > 1 or states.size < 1 or not np.issubdtype(states.dtype, np.integer):
            raise ValueError("n_states must be an int or one int per class")
        if states.min() < 1 or states.max() > HMM_MAX_STATES:
            raise ValueError("n_states must lie in [1, %d]" % HMM_MAX_STATES)
        self.n_states = int(states) if states.ndim == 0 else states.astype(np.int32)
        self.n_iter, self.var_floor, self.trans_floor = int(n_iter), float(var_floor), float(trans_floor)
        if self.n_iter < 0 or not self.var_floor > 0.0 or not np.isfinite(self.var_floor):
            raise ValueError("n_iter must be >= 0 and var_floor a positive number")
        if not 0.0 < self.trans_floor < 0.5:
            raise ValueError("trans_floor must lie in (0, 0.5)")

    def fit(self, X, y, lengths=None):
        from .pipeline import HmmModelSet, HmmUpdater, hmm_uniform_segmentation
        X, n, codes = self._training_set(X, y, lengths)
        C, F = len(self.classes_), X.shape[2]
        states = np.full(C, self.n_states, np.int32) if np.ndim(self.n_states) == 0 else self.n_states
        if len(states) != C:
            raise ValueError("%d n_states for %d classes" % (len(states), C))
        Smax = int(states.max())
        order = np.argsort(codes, kind="stable")  # each class's members in training order
        start = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=C))])
        longest = np.array([n[order[start[c]:start[c + 1]]].max() for c in range(C)])
        if (longest < states).any():
            c = int(np.argmax(longest < states))
            raise ValueError("class %r has no sequence of at least n_states = %d frames" % (self.classes_[c], states[c]))
        updater = HmmUpdater(X, n, start, order, check_finite=False)
        seg = hmm_uniform_segmentation(n[order], states[codes[order]], Smax)
        zeros = np.zeros((C, Smax, F))
        stats = updater.accumulate(zeros, zeros, states, seg, np.zeros(len(order)), self.var_floor)
        model = HmmModelSet(*stats[:4], states, self.trans_floor)
        totals = []
        for _ in range(self.n_iter):
            score, new_seg = updater.align(model)
            stats = updater.accumulate(model.mean, model.var, states, new_seg, score, self.var_floor)
            totals.append(stats[4].cpu().numpy())
            model = HmmModelSet(*stats[:4], states, self.trans_floor, prev=model)
            new_seg = new_seg.cpu().numpy()
            same = np.array_equal(new_seg, seg)
            seg = new_seg
            if same:
                break
        self.model_, self.n_iter_ = model, len(totals)
        self.totals_ = np.array(totals, dtype=np.float64).reshape(len(totals), C)
        return self

    def _scores(self, X, lengths, with_labels):
        from .pipeline import hmm_score
        Xq, nq = _as_padded(X, lengths)
        if Xq.shape[2] != self.model_.shape[2]:
            raise ValueError("X has %d feature channels, the fitted models %d" % (Xq.shape[2], self.model_.shape[2]))
        return hmm_score(self.model_, self._scale(Xq, nq), nq, with_labels=with_labels, check_finite=False)

    def score_samples(self, X, lengths=None):
        """float64 [n, C]: each sequence's negative log-likelihood along its best state path under each
        class's model (+inf where the sequence has fewer frames than the model has states)."""
        return self._scores(X, lengths, False)[0].cpu().numpy()

    def kneighbors(self, X, lengths=None):
        raise NotImplementedError("an HMM classifier keeps no training sequences")

    def predict(self, X, lengths=None):
        label = self._scores(X, lengths, True)[1].cpu().numpy()
        if (label < 0).any():
            raise ValueError("sequence %d has fewer frames than every model has states" % int(np.argmax(label < 0)))
        return self.classes_[label]


class VqClassifier(SequenceClassifier):
    """One vector-quantisation codebook per class, trained by LBG binary splitting, and the label of the
    codebook with the smallest total quantisation distortion -- the cheapest of the three classical
    isolated-word recognisers at prediction time: no time alignment, one nearest-codeword search per
    frame and class.  csrc/vq.hip (dsp_vq_score, dsp_vq_assign, dsp_vq_accumulate).
    Input handling and normalisation are ``SequenceClassifier``'s.

    n_codes    codewords per codebook: a power of two in 1 .. 256.
    n_iter     Lloyd rounds per level at most (>= 1).
    eps        the split and repair offset (normalised units), added to / subtracted from every channel.
    ``fit`` runs all classes in every device call.  The one-codeword start is each class's centroid (an
    ``accumulate`` with all-zero codes and a zero previous codebook).  Then, until ``n_codes`` is reached:
    ``pipeline.vq_split``, and rounds of assign -> accumulate -> ``pipeline.vq_repair_empty``; a level ends
    when a round gives every member the codes of the round before it (never after the level's first
    round) or after ``n_iter`` rounds.  A class with fewer valid frames than ``n_codes`` raises ValueError.
    After ``fit``: codebooks_ float64 [C, K, F] (normalised units), counts_ int64 [C, K] (each cell's frames
    in the last accumulate, before the repair), totals_ float64 [rounds run, C] (row t: each class's total
    distortion under the codebook round t started from), n_iter_ the rounds run.
    ``score_samples`` is the average distortion per frame, D / n (the divide in numpy).
    No CPU path: ``fit`` and ``predict`` raise HipError without a HIP device (constructing needs none).
    """

    def __init__(self, n_codes=16, n_iter=10, eps=0.01, normalize=True):
        super().__init__(n_neighbors=1, window=None, normalize=normalize)
        from .pipeline import VQ_MAX_CODES
        if isinstance(n_codes, bool) or not isinstance(n_codes, (int, np.integer)):
            raise ValueError("n_codes must be an int")
        if not 1 <= n_codes <= VQ_MAX_CODES or n_codes & (n_codes - 1):
            raise ValueError("n_codes must be a power of two in [1, %d]" % VQ_MAX_CODES)
        self.n_codes, self.n_iter, self.eps = int(n_codes), int(n_iter), float(eps)
        if self.n_iter < 1 or not self.eps > 0.0 or not np.isfinite(self.eps):
            raise ValueError("n_iter must be >= 1 and eps a positive number")

    def fit(self, X, y, lengths=None):
        from .pipeline import VqUpdater, vq_repair_empty, vq_split
        X, n, codes = self._training_set(X, y, lengths)
        C, F = len(self.classes_), X.shape[2]
        order = np.argsort(codes, kind="stable")  # each class's members in training order
        start = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=C))])
        frames = np.bincount(codes, weights=n, minlength=C)
        if (frames < self.n_codes).any():
            c = int(np.argmax(frames < self.n_codes))
            raise ValueError("class %r has %d frames, fewer than n_codes = %d" % (self.classes_[c], frames[c], self.n_codes))
        updater = VqUpdater(X, n, start, order, check_finite=False)
        K, sizes = 1, np.ones(C, np.int32)
        stats = updater.accumulate(np.zeros((C, 1, F)), sizes, np.zeros((len(order), X.shape[1]), np.int32),
                                   np.zeros(len(order)))
        cb, cnt = _as_host(stats[0]), _as_host(stats[1]).astype(np.int64)
        totals = []
        while K < self.n_codes:
            cb, K = vq_split(cb, self.eps), 2 * K
            sizes = np.full(C, K, np.int32)
            code = None
            for _ in range(self.n_iter):
                dist, new_code = updater.assign(cb, sizes)
                stats = updater.accumulate(cb, sizes, new_code, dist)
                totals.append(_as_host(stats[3]))
                cnt = _as_host(stats[1]).astype(np.int64)
                cb, _ = vq_repair_empty(stats[0], cnt, sizes, self.eps)
                new_code = _as_host(new_code)
                same = code is not None and np.array_equal(new_code, code)
                code = new_code
                if same:
                    break
        self.codebooks_, self.counts_, self.n_iter_ = cb, cnt, len(totals)
        self.totals_ = np.array(totals, dtype=np.float64).reshape(len(totals), C)
        return self

    def _scores(self, X, lengths, with_labels):
        from .pipeline import vq_score
        Xq, nq = _as_padded(X, lengths)
        if Xq.shape[2] != self.codebooks_.shape[2]:
            raise ValueError("X has %d feature channels, the fitted codebooks %d" % (Xq.shape[2], self.codebooks_.shape[2]))
        sizes = np.full(len(self.codebooks_), self.codebooks_.shape[1], np.int32)
        return vq_score(self.codebooks_, sizes, self._scale(Xq, nq), nq, with_labels=with_labels, check_finite=False), nq

    def score_samples(self, X, lengths=None):
        """float64 [n, C]: each sequence's average distortion per frame under each class's codebook."""
        (score, _), nq = self._scores(X, lengths, False)
        return score.cpu().numpy() / nq.astype(np.float64)[:, None]

    def kneighbors(self, X, lengths=None):
        raise NotImplementedError("a VQ classifier keeps no training sequences")

    def predict(self, X, lengths=None):
        (_, label), _ = self._scores(X, lengths, True)
        return self.classes_[label.cpu().numpy()]


class DiscreteHmmClassifier(SequenceClassifier):
    """One left-to-right HMM with discrete observations per class over ONE shared vector-quantisation
    codebook: the frames are quantised once (``pipeline.VqTokenizer``), every state emits symbols with a
    probability table, and the models are trained by Viterbi re-estimation -- integer counts, so the
    statistics need no summation order.  csrc/dhmm.hip (dsp_dhmm_score, dsp_dhmm_align,
    dsp_dhmm_accumulate).  Input handling and normalisation are ``SequenceClassifier``'s.

    n_states     states per model: an int, or one value per class (sorted class values), each in 1 .. 32.
    n_codes      codewords of the shared codebook, the alphabet: a power of two in 1 .. 256.
    n_iter       rounds of align -> accumulate -> rebuild after the uniform start; training stops early
                 when a round changes no segment boundary.
    alpha        the additive smoothing of the emission tables (> 0), see ``pipeline.DhmmModelSet``.
    trans_floor  p_stay is clamped to [trans_floor, 1 - trans_floor].
    vq_iter, eps the tokeniser's Lloyd rounds per level and its split offset (``VqClassifier``'s n_iter, eps).
    training     'viterbi' (hard counts along the best path, the default) or 'baum_welch': soft counts, the
                 state posteriors of the forward-backward pass (csrc/dhmm_fb.hip, dsp_dhmm_expect, DESIGN.md
                 §4.16).  After the same uniform start, exactly ``n_iter`` rounds of expect -> rebuild
                 (``pipeline.DhmmProbSet``); there is no early stop.
    scoring      'viterbi' (the best path's cost, the default) or 'forward': the likelihood summed over all
                 paths (dsp_dhmm_forward); ``score_samples`` then returns ``pipeline.dhmm_nll`` and ``predict``
                 the label the device decides by exact comparison.  ``decode`` always uses ``model_``.
    ``fit``: the training set, the tokeniser's fit and transform on the scaled training set, the uniform
    segmentation, one accumulate, then the rounds.  A training sequence shorter than its class's n_states
    is left out of that class's statistics; a class none of whose members is long enough raises ValueError.
    ``predict`` raises ValueError for a query with fewer frames than every model has states
    (``score_samples`` returns its row of +inf).
    After ``fit``: tokenizer_ (``pipeline.VqTokenizer``), model_ (``pipeline.DhmmModelSet``: emit, stay, adv,
    n_states), totals_ float64 [rounds run, C], n_iter_ the rounds run.  With training='baum_welch' or
    scoring='forward' also prob_ (``pipeline.DhmmProbSet``); Baum-Welch training sets model_ =
    prob_.to_costs() and totals_ to the per-class sums of ``dhmm_nll`` over the members with a non-zero
    likelihood, added in list order on the host; after Viterbi training prob_ is built from the same counts as
    model_ round by round by ``DhmmProbSet``'s formulas (``prev=`` included), so it holds the same models.
    ``fit_connected`` trains the same models from connected utterances and their transcripts instead of
    isolated clips, and ``align`` places a known word sequence in an utterance (csrc/dhmm_force.hip, DESIGN.md
    §4.18); after ``fit_connected`` totals_ is float64 [rounds run].
    No CPU path: ``fit`` and ``predict`` raise HipError without a HIP device (constructing needs none).
    """

    def __init__(self, n_states=5, n_codes=64, n_iter=10, alpha=0.5, trans_floor=1e-3, vq_iter=10, eps=0.01,
                 normalize=True, training='viterbi', scoring='viterbi'):
        super().__init__(n_neighbors=1, window=None, normalize=normalize)
        from .pipeline import HMM_MAX_STATES, VqTokenizer
        if training not in ('viterbi', 'baum_welch'):
            raise ValueError("training must be 'viterbi' or 'baum_welch', got %r" % (training,))
        if scoring not in ('viterbi', 'forward'):
            raise ValueError("scoring must be 'viterbi' or 'forward', got %r" % (scoring,))
        self.training, self.scoring = training, scoring
        states = np.asarray(n_states)
        if states.ndim > 1 or states.size < 1 or not np.issubdtype(states.dtype, np.integer):
            raise ValueError("n_states must be an int or one int per class")
        if states.min() < 1 or states.max() > HMM_MAX_STATES:
            raise ValueError("n_states must lie in [1, %d]" % HMM_MAX_STATES)
        self.n_states = int(states) if states.ndim == 0 else states.astype(np.int32)
        VqTokenizer(n_codes, vq_iter, eps)  # its argument checks
        self.n_codes, self.vq_iter, self.eps = int(n_codes), int(vq_iter), float(eps)
        self.n_iter, self.alpha, self.trans_floor = int(n_iter), float(alpha), float(trans_floor)
        if self.n_iter < 0 or not self.alpha > 0.0 or not np.isfinite(self.alpha):
            raise ValueError("n_iter must be >= 0 and alpha a positive number")
        if not 0.0 < self.trans_floor < 0.5:
            raise ValueError("trans_floor must lie in (0, 0.5)")

    def fit(self, X, y, lengths=None):
        from .pipeline import (DhmmModelSet, DhmmProbSet, DhmmUpdater, VqTokenizer, dhmm_nll,
                               hmm_uniform_segmentation)
        X, n, codes = self._training_set(X, y, lengths)
        C, K = len(self.classes_), self.n_codes
        states = np.full(C, self.n_states, np.int32) if np.ndim(self.n_states) == 0 else self.n_states
        if len(states) != C:
            raise ValueError("%d n_states for %d classes" % (len(states), C))
        Smax = int(states.max())
        order = np.argsort(codes, kind="stable")  # each class's members in training order
        start = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=C))])
        longest = np.array([n[order[start[c]:start[c + 1]]].max() for c in range(C)])
        if (longest < states).any():
            c = int(np.argmax(longest < states))
            raise ValueError("class %r has no sequence of at least n_states = %d frames" % (self.classes_[c], states[c]))
        self.tokenizer_ = VqTokenizer(K, self.vq_iter, self.eps).fit(X, n)
        updater = DhmmUpdater(self.tokenizer_.transform(X, n), n, start, order)
        seg = hmm_uniform_segmentation(n[order], states[codes[order]], Smax)
        stats = updater.accumulate(states, K, seg, np.zeros(len(order)))
        if self.training == 'baum_welch':
            prob = DhmmProbSet(stats[0], stats[2], states, self.alpha, self.trans_floor)
            totals = np.zeros((self.n_iter, C))
            for it in range(self.n_iter):
                mant, expo, occ_emit, n_valid = updater.expect(prob)
                nll = dhmm_nll(mant, expo)
                for c in range(C):  # list order, from 0.0
                    for v in nll[start[c]:start[c + 1]]:
                        if v < np.inf:
                            totals[it, c] += v
                prob = DhmmProbSet(occ_emit, n_valid, states, self.alpha, self.trans_floor, prev=prob)
            self.prob_, self.model_, self.n_iter_, self.totals_ = prob, prob.to_costs(), self.n_iter, totals
            return self
        model = DhmmModelSet(*stats[:3], states, self.alpha, self.trans_floor)
        forward = self.scoring == 'forward'  # then prob_ follows model_ round by round, prev= included
        prob = DhmmProbSet(stats[0], stats[2], states, self.alpha, self.trans_floor) if forward else None
        totals = []
        for _ in range(self.n_iter):
            score, new_seg = updater.align(model)
            stats = updater.accumulate(states, K, new_seg, score)
            totals.append(stats[3].cpu().numpy())
            model = DhmmModelSet(*stats[:3], states, self.alpha, self.trans_floor, prev=model)
            if forward:
                prob = DhmmProbSet(stats[0], stats[2], states, self.alpha, self.trans_floor, prev=prob)
            new_seg = new_seg.cpu().numpy()
            same = np.array_equal(new_seg, seg)
            seg = new_seg
            if same:
                break
        self.model_, self.n_iter_ = model, len(totals)
        self.totals_ = np.array(totals, dtype=np.float64).reshape(len(totals), C)
        if forward:
            self.prob_ = prob
        return self

    def _scores(self, X, lengths, with_labels):
        from .pipeline import dhmm_forward, dhmm_score
        Xq, nq = _as_padded(X, lengths)
        if Xq.shape[2] != self.tokenizer_.codebook_.shape[1]:
            raise ValueError("X has %d feature channels, the fitted codebook %d"
                             % (Xq.shape[2], self.tokenizer_.codebook_.shape[1]))
        sym = self.tokenizer_.transform(self._scale(Xq, nq), nq)
        if self.scoring == 'forward':
            out = dhmm_forward(self.prob_, sym, nq, with_labels=with_labels)
            return (out[0], out[1]), (out[2] if with_labels else None)
        return dhmm_score(self.model_, sym, nq, with_labels=with_labels)

    def score_samples(self, X, lengths=None):
        """float64 [n, C]: each sequence's negative log-likelihood under each class's model, along its best
        state path (scoring='viterbi') or summed over all paths (scoring='forward'); +inf where the sequence
        has fewer frames than the model has states."""
        from .pipeline import dhmm_nll
        score = self._scores(X, lengths, False)[0]
        return dhmm_nll(*score) if self.scoring == 'forward' else score.cpu().numpy()

    def kneighbors(self, X, lengths=None):
        raise NotImplementedError("an HMM classifier keeps no training sequences")

    def predict(self, X, lengths=None):
        label = self._scores(X, lengths, True)[1].cpu().numpy()
        if (label < 0).any():
            raise ValueError("sequence %d has fewer frames than every model has states" % int(np.argmax(label < 0)))
        return self.classes_[label]

    def decode(self, X, lengths=None, word_penalty=0.0, max_words=None, grammar=None):
        """Connected words: each utterance of X is several words in a row with unknown boundaries, decoded by
        the one-pass Viterbi over a loop of the class models (csrc/dhmm_decode.hip, dsp_dhmm_decode, DESIGN.md
        §4.15; at most ``pipeline.DHMM_DECODE_MAX_MODELS`` classes).  The frames are tokenised exactly as
        ``predict`` does.  ``word_penalty``: the cost of starting a word, a scalar or one value per class.
        ``grammar``: None for the free loop -- any word after any word -- or a ``WordPairGrammar`` over the
        indices of ``classes_``: the words are then decoded under its costs with the penalty added through
        ``grammar.plus(word_penalty)`` (csrc/dhmm_grammar.hip, dsp_dhmm_decode_grammar; that
        call has no ``cum`` output, which this method never returned).
        Returns (labels, starts): per utterance the class labels of its words in time order and their first
        frames, both empty for an utterance no word sequence fits."""
        from .pipeline import dhmm_decode, dhmm_decode_grammar
        Xq, nq = self._symbols(X, lengths)
        sym = self.tokenizer_.transform(self._scale(Xq, nq), nq)
        if grammar is None:
            _, n_words, words, start, _ = dhmm_decode(self.model_, sym, nq, enter=word_penalty, max_words=max_words)
        else:
            if grammar.n_classes != len(self.classes_):
                raise ValueError("the grammar has %d words, the classifier %d classes" % (grammar.n_classes, len(self.classes_)))
            g = grammar.plus(word_penalty)
            _, n_words, words, start = dhmm_decode_grammar(self.model_, sym, nq, g.enter, g.pair, g.leave, max_words=max_words)
        n_words, words, start = (t.cpu().numpy() for t in (n_words, words, start))
        kept = np.minimum(n_words, words.shape[1])
        return ([self.classes_[words[i, :kept[i]]] for i in range(len(kept))],
                [start[i, :kept[i]].copy() for i in range(len(kept))])

    def _transcript_codes(self, transcripts, N):
        """The transcripts' labels as indices into ``classes_``: (trans int32 [N, Wmax], n_trans int32 [N])."""
        from .pipeline import _dhmm_transcripts
        if len(transcripts) != N:
            raise ValueError("%d transcripts for %d utterances" % (len(transcripts), N))
        rows = []
        for r in transcripts:
            r = np.asarray(r).reshape(-1)
            at = np.searchsorted(self.classes_, r) if len(r) else np.zeros(0, np.int64)
            at = np.minimum(at, len(self.classes_) - 1)
            if len(r) and (self.classes_[at] != r).any():
                raise ValueError("transcript label %r is not one of the fitted classes" % (r[self.classes_[at] != r][0],))
            rows.append(at)
        return _dhmm_transcripts(rows, None, N)

    def _symbols(self, X, lengths):
        """The padded utterances of ``decode`` and ``align``, checked against the fitted codebook's channels."""
        Xq, nq = _as_padded(X, lengths)
        if Xq.shape[2] != self.tokenizer_.codebook_.shape[1]:
            raise ValueError("X has %d feature channels, the fitted codebook %d"
                             % (Xq.shape[2], self.tokenizer_.codebook_.shape[1]))
        return Xq, nq

    def align(self, X, transcripts, lengths=None, word_penalty=0.0):
        """Forced alignment: where are the words of each utterance's KNOWN word sequence?  Every utterance is
        aligned against the concatenation of its transcript's class models (csrc/dhmm_force.hip,
        dsp_dhmm_force_align; at most ``pipeline.DHMM_FORCE_MAX_WORDS`` words a transcript).
        The frames are tokenised exactly as ``decode`` does; ``word_penalty`` is ``decode``'s.  ``transcripts``:
        per utterance the sequence of its words' class labels; a label not in ``classes_`` raises ValueError.
        Returns (starts, scores): per utterance the first frame of each transcript word, and the forced score
        float64 [n]; an utterance the transcript does not fit gets empty starts and a score of +inf."""
        from .pipeline import dhmm_force_align
        Xq, nq = self._symbols(X, lengths)
        trans, n_trans = self._transcript_codes(transcripts, len(nq))
        sym = self.tokenizer_.transform(self._scale(Xq, nq), nq)
        score, seg = dhmm_force_align(self.model_, sym, nq, trans, enter=word_penalty, n_trans=n_trans)
        score, first = score.cpu().numpy(), seg[:, :, 0].cpu().numpy()
        return [first[i, :n_trans[i]].copy() if score[i] < np.inf else np.zeros(0, np.int32) for i in range(len(nq))], score

    def fit_connected(self, X, transcripts, lengths=None, word_penalty=0.0):
        """Embedded Viterbi training from connected utterances and their transcripts -- no word boundary is
        marked by hand (csrc/dhmm_force.hip).  ``classes_`` becomes the sorted labels of all
        transcripts (at most ``pipeline.DHMM_DECODE_MAX_MODELS``); normalisation and the tokeniser are fitted on
        all utterance frames; the flat start (``pipeline.dhmm_flat_segmentation``) and one accumulate give the
        first models; then up to ``n_iter`` rounds of align -> accumulate -> rebuild
        (``DhmmModelSet(..., prev=model)``), stopping early when a round changes no entry of seg.  An utterance
        shorter than its chain of states is left out; a word with no instance in any utterance that is long
        enough raises ValueError, as does training='baum_welch' (there is no embedded forward-backward).
        After the fit: tokenizer_, model_, n_iter_, totals_ float64 [rounds]: per round the forced scores of the
        valid utterances added in utterance order on the host; with scoring='forward' also prob_, built from the
        same counts as in ``fit``."""
        from .pipeline import (DHMM_DECODE_MAX_MODELS, DhmmForceUpdater, DhmmModelSet, DhmmProbSet, VqTokenizer,
                               dhmm_flat_segmentation)
        if self.training == 'baum_welch':
            raise ValueError("fit_connected trains by Viterbi re-estimation: there is no embedded Baum-Welch")
        X, n = _as_padded(X, lengths)
        if len(transcripts) != len(X):
            raise ValueError("%d transcripts for %d utterances" % (len(transcripts), len(X)))
        words = [np.asarray(r).reshape(-1) for r in transcripts]
        if any(len(r) < 1 for r in words):
            raise ValueError("empty transcript at index %d" % [len(r) < 1 for r in words].index(True))
        self.classes_ = np.unique(np.concatenate(words))
        C, K = len(self.classes_), self.n_codes
        if C > DHMM_DECODE_MAX_MODELS:
            raise ValueError("fit_connected takes at most %d word classes, got %d" % (DHMM_DECODE_MAX_MODELS, C))
        states = np.full(C, self.n_states, np.int32) if np.ndim(self.n_states) == 0 else self.n_states
        if len(states) != C:
            raise ValueError("%d n_states for %d classes" % (len(states), C))
        trans, n_trans = self._transcript_codes(words, len(X))
        Smax = int(states.max())
        if self.normalize:
            frames = X[np.arange(X.shape[1])[None, :] < n[:, None]]  # all valid frames, as _training_set
            self.mean_ = np.mean(frames, axis=0)
            std = np.std(frames, axis=0)
            self.std_ = np.where(std == 0, 1.0, std)
        X = self._scale(X, n)
        self.tokenizer_ = VqTokenizer(K, self.vq_iter, self.eps).fit(X, n)
        updater = DhmmForceUpdater(self.tokenizer_.transform(X, n), n, trans, n_trans)
        seg = dhmm_flat_segmentation(n, trans, n_trans, states, Smax)
        stats = updater.accumulate(states, K, seg)
        n_valid = stats[2].cpu().numpy()
        if (n_valid == 0).any():
            c = int(np.argmin(n_valid))
            raise ValueError("class %r has no instance in an utterance of at least as many frames as its transcript "
                             "has states" % (self.classes_[c],))
        model = DhmmModelSet(*stats[:3], states, self.alpha, self.trans_floor)
        forward = self.scoring == 'forward'  # then prob_ follows model_ round by round, prev= included
        prob = DhmmProbSet(stats[0], stats[2], states, self.alpha, self.trans_floor) if forward else None
        totals = []
        for _ in range(self.n_iter):
            score, new_seg = updater.align(model, word_penalty)
            stats = updater.accumulate(states, K, new_seg)
            kept = score.cpu().numpy()[stats[3].cpu().numpy() != 0]
            totals.append(np.cumsum(kept)[-1] if len(kept) else 0.0)  # sequential, utterance order: np.sum adds pairwise
            model = DhmmModelSet(*stats[:3], states, self.alpha, self.trans_floor, prev=model)
            if forward:
                prob = DhmmProbSet(stats[0], stats[2], states, self.alpha, self.trans_floor, prev=prob)
            new_seg = new_seg.cpu().numpy()
            same = np.array_equal(new_seg, seg)
            seg = new_seg
            if same:
                break
        self.model_, self.n_iter_, self.totals_ = model, len(totals), np.array(totals, dtype=np.float64)
        if forward:
            self.prob_ = prob
        self._index = None
        return self


class WordPairGrammar:
    """The costs of a word-pair grammar for ``DiscreteHmmClassifier.decode(grammar=...)`` and
    ``pipeline.dhmm_decode_grammar`` (csrc/dhmm_grammar.hip), host only.  Words are indices
    into the classifier's ``classes_``.  ``enter`` float64 [C]: the cost of starting an utterance with each
    word; ``pair`` float64 [C, C]: pair[p, c] the cost of word c following word p; ``leave`` float64 [C]: the
    cost of ending an utterance on each word.  Finite or +inf; +inf forbids."""

    def __init__(self, enter, pair, leave):
        self.pair = np.array(pair, np.float64)
        C = self.pair.shape[0]
        if self.pair.shape != (C, C) or C < 1:
            raise ValueError("pair must be [C, C], got shape %s" % (self.pair.shape,))
        self.enter = np.zeros(C) if enter is None else np.array(np.broadcast_to(np.asarray(enter, np.float64), (C,)))
        self.leave = np.zeros(C) if leave is None else np.array(np.broadcast_to(np.asarray(leave, np.float64), (C,)))
        for name in ("enter", "pair", "leave"):
            v = getattr(self, name)
            if np.isnan(v).any() or (v == -np.inf).any():
                raise ValueError("%s must be finite or +inf" % name)

    @property
    def n_classes(self):
        return self.pair.shape[0]

    @classmethod
    def from_transcripts(cls, transcripts, n_classes, alpha=0.5):
        """Add-alpha bigram estimates with a sentence-end event from word-index sequences (empty ones are
        skipped): with U utterances, first[c] of them starting with c, n[p, c] bigrams and end[p] utterances
        ending on p,
            enter[c]   = -log((first[c] + alpha) / (U + alpha C))
            pair[p, c] = -log((n[p, c] + alpha) / (sum_c n[p, c] + end[p] + alpha (C + 1)))
            leave[p]   = -log((end[p]  + alpha) / (sum_c n[p, c] + end[p] + alpha (C + 1)))
        in fp64 with numpy's logarithm.  With alpha = 0 an unseen event costs +inf."""
        C, alpha = int(n_classes), np.float64(alpha)
        if C < 1 or not alpha >= 0:
            raise ValueError("n_classes >= 1 and alpha >= 0")
        first, n, end = np.zeros(C), np.zeros((C, C)), np.zeros(C)
        U = 0
        for r in transcripts:
            r = np.asarray(r).astype(np.int64).reshape(-1)
            if not len(r):
                continue
            if r.min() < 0 or r.max() >= C:
                raise ValueError("a transcript word lies outside [0, %d)" % C)
            U += 1
            first[r[0]] += 1
            end[r[-1]] += 1
            np.add.at(n, (r[:-1], r[1:]), 1)

        def cost(count, total):
            num = count + alpha
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.where(num > 0, -np.log(num / total), np.inf)

        row = n.sum(axis=1) + end + alpha * np.float64(C + 1)
        return cls(cost(first, np.float64(U) + alpha * np.float64(C)), cost(n, row[:, None]), cost(end, row))

    @classmethod
    def from_allowed(cls, follows, first=None, last=None):
        """A finite-state syntax: ``follows`` bool [C, C] (word c may follow word p), ``first`` / ``last`` bool
        [C] (may start / end an utterance; None: every word may).  Allowed costs 0.0, forbidden +inf."""
        follows = np.asarray(follows, bool)
        C = follows.shape[0]
        flag = lambda a: np.ones(C, bool) if a is None else np.asarray(a, bool).reshape(C)
        price = lambda a: np.where(a, 0.0, np.inf)
        return cls(price(flag(first)), price(follows), price(flag(last)))

    def plus(self, word_penalty):
        """The grammar with a word penalty (a scalar or one value per word: the cost of starting that word) added
        to ``enter`` and to every row of ``pair``, in fp64."""
        pen = np.array(np.broadcast_to(np.asarray(word_penalty, np.float64), (self.n_classes,)))
        return WordPairGrammar(self.enter + pen, self.pair + pen[None, :], self.leave)


def word_error_rate(ref, hyp):
    """(substitutions + deletions + insertions) / reference words over paired lists of label sequences: the
    plain Levenshtein distance of each pair, summed, over the summed reference lengths (host only)."""
    if len(ref) != len(hyp):
        raise ValueError("%d reference sequences for %d hypotheses" % (len(ref), len(hyp)))
    errors = total = 0
    for r, h in zip(ref, hyp):
        r, h = list(r), list(h)
        row = list(range(len(h) + 1))
        for i in range(1, len(r) + 1):
            diag, row[0] = row[0], i
            for j in range(1, len(h) + 1):
                diag, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, diag + (r[i - 1] != h[j - 1]))
        errors += row[len(h)]
        total += len(r)
    if total == 0:
        raise ValueError("the reference holds no word")
    return errors / total


# ==================== MLP (models.py:77-221) ====================

def _build_network(input_size, hidden_layers, num_classes, dropout):
    """MLPClassifier.network (models.py:90-103): Linear / ReLU / Dropout per hidden layer, a last Linear."""
    from torch import nn
    layers, prev = [], int(input_size)
    for h in hidden_layers:
        layers += [nn.Linear(prev, int(h)), nn.ReLU(), nn.Dropout(dropout)]
        prev = int(h)
    layers.append(nn.Linear(prev, int(num_classes)))
    return nn.Sequential(*layers)


def _pack(network):
    """The packed buffer of include/dsp_audiorec.h: the state_dict's tensors in order, flattened."""
    import torch
    return torch.cat([t.detach().reshape(-1).to(torch.float32) for t in network.state_dict().values()])


def _unpack(network, packed):
    import torch
    sd, off = network.state_dict(), 0
    with torch.no_grad():
        for t in sd.values():
            t.copy_(packed[off:off + t.numel()].reshape(t.shape))
            off += t.numel()
    return network


class MLPTrainer:
    """models.py:109-221: fit / predict / evaluate, train_losses / train_accuracies, the reference's
    result keys.  The initial weights are nn.Linear's default init of the reference's module.

    Extensions (keywords after ``device``; the reference has none of them):
      seed     None: weights from torch's global RNG as in the reference, and a seed for the shuffle
               and the dropout drawn from it.  An int makes init, shuffle and dropout reproducible
               without touching the global RNG.
      dropout  the reference's fixed 0.3 (MLPClassifier's default).
      backend  'fused': csrc/mlp.hip, the whole training loop in one persistent workgroup
               (dsp_mlp_train) and dsp_mlp_predict; raises outside its plan (dsp_mlp_lds_bytes == 0).
               'torch': the reference's loop in plain torch on the ROCm device (any shape; also
               the baseline of tools/mlp_bench.py).  'auto': fused inside its plan, torch outside.
    No CPU path: ``fit`` raises HipError without a HIP device (constructing needs none).
    """

    EPOCH_CHUNK_BYTES = 64 << 20  # bound on one launch's shuffle orders (perm int32 [epochs, N])

    def __init__(self, input_size, hidden_layers, num_classes, learning_rate=0.001, epochs=100, batch_size=16,
                 device=None, seed=None, dropout=0.3, backend='auto'):
        import torch
        if backend not in ('auto', 'fused', 'torch'):
            raise ValueError("backend must be 'auto', 'fused' or 'torch'")
        self.input_size, self.hidden_layers = int(input_size), [int(h) for h in hidden_layers]
        self.num_classes, self.learning_rate = int(num_classes), float(learning_rate)
        self.epochs, self.batch_size = int(epochs), int(batch_size)
        self.device, self.dropout, self.backend = device, float(dropout), backend
        if seed is None:
            network = _build_network(input_size, self.hidden_layers, num_classes, self.dropout)
            self.seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        else:
            self.seed = int(seed)
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(self.seed)
                network = _build_network(input_size, self.hidden_layers, num_classes, self.dropout)
        self._network = network      # 'torch' backend: the live module (moved to the device at fit)
        self._params = _pack(network)  # 'fused' backend: packed parameters (on the device after fit)
        self._m = self._v = self._optimizer = self._gen = None
        self._steps = 0
        self._pending = []
        self._fused = None  # decided at the first fit
        self.train_losses = []
        self.train_accuracies = []

    # -- backend choice ---------------------------------------------------------------------
    def _use_fused(self):
        if self._fused is None:
            from .pipeline import mlp_lds_bytes
            inside = self.backend != 'torch' and mlp_lds_bytes(self.input_size, self.hidden_layers,
                                                               self.num_classes, self.batch_size) > 0
            if self.backend == 'fused' and not inside:
                raise ValueError("MLP shape outside the fused kernel's plan (dsp_mlp_lds_bytes == 0): "
                                 "use backend='torch' or 'auto'")
            self._fused = inside
        return self._fused

    def _device(self):
        from . import _hip
        d = _hip.require_device()
        if self.device is not None:
            import torch
            d = torch.device(self.device)
            if d.type != 'cuda':
                raise _hip.HipError("the MLP trains only on a HIP device, not on %s" % d)
        return d

    def _generator(self, d):
        import torch
        if self._gen is None:
            self._gen = torch.Generator(device=d)
            self._gen.manual_seed(self.seed)
        return self._gen

    @property
    def model(self):
        """The equivalent nn.Sequential (Linear/ReLU/Dropout ... Linear) with the current weights."""
        if self._fused:
            net = _build_network(self.input_size, self.hidden_layers, self.num_classes, self.dropout)
            return _unpack(net, self._params).to(self._params.device).eval()  # a snapshot
        return self._network

    # -- training ---------------------------------------------------------------------------
    def fit(self, X_train, y_train, verbose=True):
        d = self._device()
        if self._use_fused():
            _fit_fused([self], X_train, y_train, d, verbose)
        else:
            self._fit_torch(X_train, y_train, d, verbose)
        return self

    def _log(self, first, verbose):
        if verbose:
            for e in range(first, len(self.train_losses)):
                if (e + 1) % 10 == 0:
                    print(f'Epoch [{e + 1}/{self.epochs}], Loss: {self.train_losses[e]:.4f}, '
                          f'Accuracy: {self.train_accuracies[e]:.4f}')

    def _flush(self, verbose):
        """Histories of finished launches (device tensors until here) into the Python lists."""
        first = len(self.train_losses)
        for loss, acc in self._pending:
            self.train_losses += [float(x) for x in loss.cpu().tolist()]
            self.train_accuracies += [float(x) for x in acc.cpu().tolist()]
        self._pending = []
        self._log(first, verbose)

    def _fit_torch(self, X_train, y_train, d, verbose):
        """models.py:146-194 as written, on the device: one optimizer step per batch, one
        loss.item() per step.  The shuffle is this trainer's generator, the dropout the device's."""
        import torch
        from torch import nn, optim
        X = torch.as_tensor(np.asarray(X_train), dtype=torch.float32).to(d)
        y = torch.as_tensor(np.asarray(y_train), dtype=torch.int64).to(d)
        net = self._network.to(d)
        if self._optimizer is None:
            self._optimizer = optim.Adam(net.parameters(), lr=self.learning_rate)
        criterion, gen, N = nn.CrossEntropyLoss(), self._generator(d), X.shape[0]
        with torch.random.fork_rng(devices=[d]):
            torch.manual_seed(self.seed + self._steps)
            net.train()
            for _ in range(self.epochs):
                order = torch.randperm(N, generator=gen, device=d)
                epoch_loss, correct, total, nb = 0.0, 0, 0, 0
                for lo in range(0, N, self.batch_size):
                    idx = order[lo:lo + self.batch_size]
                    batch_X, batch_y = X[idx], y[idx]
                    outputs = net(batch_X)
                    loss = criterion(outputs, batch_y)
                    self._optimizer.zero_grad()
                    loss.backward()
                    self._optimizer.step()
                    epoch_loss += loss.item()
                    _, predicted = torch.max(outputs.data, 1)
                    total += batch_y.size(0)
                    correct += (predicted == batch_y).sum().item()
                    nb += 1
                    self._steps += 1
                self.train_losses.append(epoch_loss / nb)
                self.train_accuracies.append(correct / total)
                self._log(len(self.train_losses) - 1, verbose)

    def predict(self, X_test):
        import torch
        if self._fused:
            from .pipeline import mlp_predict
            pred, _ = mlp_predict(self._params, np.asarray(X_test, dtype=np.float32), self.hidden_layers,
                                  self.num_classes)
            return pred.cpu().numpy().astype(np.int64)
        d = self._device()
        net = self._network.to(d)
        net.eval()
        with torch.no_grad():
            outputs = net(torch.as_tensor(np.asarray(X_test), dtype=torch.float32).to(d))
            _, predicted = torch.max(outputs.data, 1)
        return predicted.cpu().numpy()

    def evaluate(self, X_test, y_test):
        from sklearn.metrics import accuracy_score, classification_report, confusion_matrix
        y_pred = self.predict(X_test)
        return {
            'accuracy': accuracy_score(y_test, y_pred),
            'predictions': y_pred,
            'classification_report': classification_report(y_test, y_pred, output_dict=True, zero_division=0),
            'confusion_matrix': confusion_matrix(y_test, y_pred),
            'train_losses': self.train_losses,
            'train_accuracies': self.train_accuracies,
        }


def _fit_fused(trainers, X_train, y_train, d, verbose):
    """The trainers' epochs in launches of dsp_mlp_train, one workgroup per trainer.  Every trainer
    keeps its own shuffle generator, so a model trains the same alone or in a batch."""
    import torch
    from .pipeline import mlp_train
    t0 = trainers[0]
    # a list of arrays: one training set per trainer, all of the same shape (else one shared set)
    X = torch.as_tensor(np.asarray(X_train), dtype=torch.float32).to(d).contiguous()
    y = torch.as_tensor(np.asarray(y_train)).to(device=d, dtype=torch.int32).contiguous()
    N, K = X.shape[-2], len(trainers)
    if X.shape[-1] != t0.input_size or X.dim() != (3 if isinstance(X_train, (list, tuple)) else 2):
        raise ValueError("X of shape %s does not fit %d models of %d features" % (tuple(X.shape), K, t0.input_size))
    P = t0._params.numel()
    params = torch.stack([t._params.to(d) for t in trainers]).contiguous()
    zeros = torch.zeros(P, dtype=torch.float32, device=d)
    m = torch.stack([zeros if t._m is None else t._m for t in trainers]).contiguous()
    v = torch.stack([zeros if t._v is None else t._v for t in trainers]).contiguous()
    steps = torch.tensor([t._steps for t in trainers], dtype=torch.int64, device=d)
    lr = torch.tensor([t.learning_rate for t in trainers], dtype=torch.float64, device=d)
    seeds = torch.as_tensor(np.array([t.seed & 0xFFFFFFFF for t in trainers], dtype=np.uint32).view(np.int32)).to(d)
    gens = [t._generator(d) for t in trainers]
    chunk = max(1, min(t0.epochs, MLPTrainer.EPOCH_CHUNK_BYTES // (4 * N * K)))
    if verbose:
        chunk = min(chunk, 10)  # the reference's every-10-epochs line appears as training goes
    done = 0
    while done < t0.epochs:
        ne = min(chunk, t0.epochs - done)
        perm = torch.stack([torch.stack([torch.randperm(N, generator=g, device=d, dtype=torch.int32)
                                         for _ in range(ne)]) for g in gens]).contiguous()
        loss, acc = mlp_train(X, y, t0.hidden_layers, t0.num_classes, perm, params, m, v, steps, lr, seeds,
                              t0.batch_size, dropout=t0.dropout, perm_stride=ne * N if K > 1 else 0)
        if verbose:
            loss, acc = loss.cpu(), acc.cpu()
        for k, t in enumerate(trainers):
            t._pending.append((loss[k], acc[k]))
            if verbose:
                t._flush(K == 1)
        done += ne
    nb = (N + t0.batch_size - 1) // t0.batch_size
    for k, t in enumerate(trainers):
        t._params, t._m, t._v = params[k].clone(), m[k].clone(), v[k].clone()
        t._steps += t0.epochs * nb
        t._flush(False)


def fit_mlp_models(X_train, y_train, input_size, hidden_layers, num_classes, learning_rates, seeds=None,
                   epochs=100, batch_size=16, dropout=0.3, verbose=False):
    """Train one MLP per learning rate (and seed) in ONE dsp_mlp_train launch per epoch chunk -- a
    workgroup per model -- and return the fitted MLPTrainers.  Model k equals
    ``MLPTrainer(..., learning_rate=learning_rates[k], seed=seeds[k], backend='fused').fit(X, y)``
    bit for bit.  (Extension: the reference trains such sweeps one model after another.)"""
    from . import _hip
    seeds = list(range(len(learning_rates))) if seeds is None else list(seeds)
    if len(seeds) != len(learning_rates):
        raise ValueError("one seed per learning rate")
    trainers = [MLPTrainer(input_size, hidden_layers, num_classes, learning_rate=lr, epochs=epochs,
                           batch_size=batch_size, seed=s, dropout=dropout, backend='fused')
                for lr, s in zip(learning_rates, seeds)]
    if not trainers:
        return trainers
    d = _hip.require_device()
    for t in trainers:
        t._use_fused()
    _fit_fused(trainers, X_train, y_train, d, verbose)
    return trainers


def create_classifier(classifier_type, **kwargs):
    """models.py:226-246.  'mlp' takes MLPTrainer's arguments; 'dtw_knn', 'dtw_template', 'hmm', 'vq' and 'dhmm' (extensions) are
    the SequenceClassifier, the TemplateClassifier, the HmmClassifier, the VqClassifier and the DiscreteHmmClassifier.  A bare ``create_classifier('mlp')``
    raises NotImplementedError naming them (the reference fails there with a TypeError)."""
    if classifier_type in ['knn', 'naive_bayes', 'decision_tree', 'svm']:
        return TraditionalClassifier(classifier_type, **kwargs)
    if classifier_type == 'dtw_knn':
        return SequenceClassifier(**kwargs)
    if classifier_type == 'dtw_template':
        return TemplateClassifier(**kwargs)
    if classifier_type == 'hmm':
        return HmmClassifier(**kwargs)
    if classifier_type == 'vq':
        return VqClassifier(**kwargs)
    if classifier_type == 'dhmm':
        return DiscreteHmmClassifier(**kwargs)
    if classifier_type == 'mlp':
        if not kwargs:
            raise NotImplementedError("create_classifier('mlp') needs input_size, hidden_layers and num_classes "
                                      "(MLPTrainer's required arguments, models.py:112-114)")
        return MLPTrainer(**kwargs)
    raise ValueError(f"不支持的分类器类型: {classifier_type}")
