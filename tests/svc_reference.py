"""numpy restatement of libsvm's SVC(kernel='rbf') predict -- the contract of dsp_svc_predict
(include/dsp_audiorec.h) -- and the derived bound on |dec_device - dec_libsvm|.

A model is a dict of libsvm's own arrays as scikit-learn keeps them (the underscore attributes):
sv [nSV, D], n_support [C], dual_coef [C-1, nSV], intercept [C(C-1)/2], gamma, classes [C].
"""
import numpy as np

EXP_ULPS = 4.0   # allowance per exp and side (csrc/svm.hip SVC_EXP_ULPS)
SAFETY = 4.0     # certified: |dec_p| > SAFETY * bound_p (csrc/svm.hip SVC_SAFETY)
INV_E = 0.36787944117144233


def model_arrays(m):
    """The arrays of a fitted sklearn.svm.SVC."""
    C = len(m.classes_)
    nSV = m.support_vectors_.shape[0]
    return dict(sv=np.ascontiguousarray(m.support_vectors_, dtype=np.float64),
                n_support=np.asarray(m._n_support, dtype=np.int32),
                dual_coef=np.ascontiguousarray(m._dual_coef_, dtype=np.float64).reshape(C - 1, nSV),
                intercept=np.asarray(m._intercept_, dtype=np.float64).reshape(C * (C - 1) // 2),
                gamma=np.float64(m._gamma), classes=np.asarray(m.classes_))


def pairs(C):
    """libsvm's pair order."""
    return [(i, j) for i in range(C) for j in range(i + 1, C)]


def kernel_values(model, X):
    X = np.asarray(X, dtype=np.float64)
    diff = X[:, None, :] - model['sv'][None, :, :]
    return np.exp(-model['gamma'] * np.sum(diff * diff, axis=2))  # [Nq, nSV]


def decision_values(model, X):
    """dec [Nq, C(C-1)/2] with libsvm's signs."""
    K = kernel_values(model, X)
    ns, coef, b = model['n_support'], model['dual_coef'], model['intercept']
    start = np.concatenate([[0], np.cumsum(ns)])
    C = len(ns)
    dec = np.empty((K.shape[0], C * (C - 1) // 2))
    for p, (i, j) in enumerate(pairs(C)):
        si, sj = slice(start[i], start[i + 1]), slice(start[j], start[j + 1])
        dec[:, p] = K[:, si] @ coef[j - 1, si] + K[:, sj] @ coef[i, sj] + b[p]
    return dec


def vote(dec, C):
    """Class index per row: a vote for i if dec_p > 0 else for j, the first class with the most."""
    votes = np.zeros((dec.shape[0], C), dtype=np.int64)
    for p, (i, j) in enumerate(pairs(C)):
        pos = dec[:, p] > 0
        votes[:, i] += pos
        votes[:, j] += ~pos
    return np.argmax(votes, axis=1)


def predict(model, X):
    return model['classes'][vote(decision_values(model, X), len(model['n_support']))]


def sklearn_signs(dec):
    """libsvm's dec as SVC.decision_function(ovo) reports it: [n] and negated for two classes."""
    return -dec.ravel() if dec.shape[1] == 1 else dec


def dec_bound(model, X):
    """bound [Nq, C(C-1)/2] on the difference between two correctly rounded fp64 evaluations of dec_p
    (any summation order, any distance order, FMA or not, an exp within EXP_ULPS ulp on each side):

      2^-52 [ (n_i + n_j + 4) (B_q + |b_p|) + 2 EXP_ULPS B_q + (D + 4) A / e ]

    B_q = sum_s K_s max_r |coef[r][s]|, A = sum_s max_r |coef[r][s]|.  Per side, with u = 2^-53:
    summing the n_i + n_j products and the intercept costs at most (n_i + n_j + 2) u of
    sum |terms| <= B_q + |b_p| (one rounding per product, one per addition, in any order); an exp
    within EXP_ULPS ulp costs 2 EXP_ULPS u K_s; the argument x = gamma d^2 carries a relative error
    of at most (D + 4) u (subtraction, square, D - 1 additions of non-negative terms, the product
    with gamma, and slack), and |d/dx e^-x| x = x e^-x <= 1/e turns that into an absolute error of
    (D + 4) u / e per K_s, whatever x is -- hence the weight A, not B_q."""
    K = kernel_values(model, X)
    cmax = np.max(np.abs(model['dual_coef']), axis=0)
    B = K @ cmax
    A = cmax.sum()
    ns, b = model['n_support'], model['intercept']
    D = model['sv'].shape[1]
    C = len(ns)
    out = np.empty((K.shape[0], C * (C - 1) // 2))
    for p, (i, j) in enumerate(pairs(C)):
        out[:, p] = 2.0 ** -52 * ((ns[i] + ns[j] + 4) * (B + abs(b[p])) + 2 * EXP_ULPS * B + (D + 4) * A * INV_E)
    return out
