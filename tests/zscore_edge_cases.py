"""Edge shapes and data of the z-score (csrc/zscore.hip), shared by the CPU check of the oracle
(tests/test_knn_edges_host.py) and the GPU tests (tests/test_gpu_zscore_edges.py); a plain helper
module.  The reference of both is numpy itself: np.mean / np.std over axis 0 of a C-contiguous
float64 array.

D: one column (numpy's pairwise order), and either side of the kernel's 16-column workgroups, the
recogniser's 15 and the sequence method's 198.  N: either side of numpy's 8-element threshold, the
kernel's 16-row batches, a 256-row tile, and an odd and an even tile count.
"""
import numpy as np

DS = (1, 2, 15, 16, 17, 31, 32, 33, 198)
NS = (1, 2, 7, 8, 9, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1000)
SPECIAL_SHAPES = ((1000, 1), (257, 15), (513, 17))
# one column past numpy's 8192-element buffer: a second chunk of 1 and of 7 rows, three chunks, and
# more leaf blocks than the kernel's one workgroup sums at once (256)
LONG_COLUMNS = (8191, 8192, 8193, 8199, 20000, 70001)


def _plain(rng, N, D):
    """Columns of different scales (0.1 .. 100) and offsets (+-50)."""
    scale = 10.0 ** rng.uniform(-1.0, 2.0, D)
    offset = rng.uniform(-50.0, 50.0, D)
    return np.ascontiguousarray(offset + scale * rng.standard_normal((N, D)))


def matrices():
    """[(name, X)]: the full D x N product, then the special matrices."""
    out = []
    for D in DS:
        for N in NS:
            out.append(("plain_N%d_D%d" % (N, D), _plain(np.random.default_rng(1000 * D + N), N, D)))
    for N, D in SPECIAL_SHAPES:
        rng = np.random.default_rng(7000 + D)
        X = _plain(rng, N, D)
        X[:, D // 2] = 3.25  # a constant column: std 0 -> 1
        out.append(("constant_column_N%d_D%d" % (N, D), X))
        X = _plain(rng, N, D)
        X[:, D - 1] = 1e9 + 0.5  # constant, its running sum inexact: whatever std numpy is left with
        out.append(("constant_1e9_column_N%d_D%d" % (N, D), X))
        out.append(("offset_1e8_N%d_D%d" % (N, D), np.ascontiguousarray(1e8 + rng.standard_normal((N, D)))))
    for N in LONG_COLUMNS:
        out.append(("long_column_N%d" % N, _plain(np.random.default_rng(N), N, 1)))
    return out
