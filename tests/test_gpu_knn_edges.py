"""The exact KNN at its numeric and shape edges (tests/knn_edge_cases.py): every case through
src.pipeline.knn_classify, indices, fp64 distances and votes equal to the C oracle's -- -1 / inf
where a query has fewer than k candidates, pred -1 where it has none -- and the fallback count
where the code implies one.  tests/test_knn_edges_host.py pins on the CPU that every case is finite
and tie-free, so equality is the only right answer."""
import numpy as np
import pytest

import knn_edge_cases as kc
import oracle

pytestmark = pytest.mark.gpu


def _run(cases):
    from src.pipeline import knn_classify
    bad, counts = [], {}
    for c in cases:
        ref, labels, query, k, self_offset = c.data()
        i0, d0, p0 = oracle.knn(ref, labels, query, k, n_classes=kc.N_CLASSES, self_offset=self_offset, nthreads=8)
        stats = {}
        i1, d1, p1 = knn_classify(ref, labels, query, k, self_offset=self_offset, stats=stats)
        i1, d1, p1 = i1.cpu().numpy(), d1.cpu().numpy(), p1.cpu().numpy()
        fb = stats.get("fallbacks", 0)  # no launch (and no count) for an empty query batch
        counts[c.name] = fb
        wrong = [n for n, a, b in (("idx", i1, i0), ("dist", d1, d0), ("pred", p1, p0)) if not np.array_equal(a, b)]
        if isinstance(c.fallbacks, tuple):
            if fb < c.fallbacks[1]:
                wrong.append("fallbacks %d < %d" % (fb, c.fallbacks[1]))
        elif c.fallbacks is not None and fb != c.fallbacks and query.shape[0] > 0:
            wrong.append("fallbacks %d != %d" % (fb, c.fallbacks))
        if wrong:
            rows = np.flatnonzero((i1 != i0).any(1) | (d1 != d0).any(1) | (p1 != p0))
            bad.append("%s/%s: %s (%d of %d queries differ, first %s)"
                       % (c.group, c.name, ", ".join(wrong), rows.size, query.shape[0], rows[:4].tolist()))
    print("fallbacks:", counts)
    assert not bad, "%d of %d cases:\n%s" % (len(bad), len(cases), "\n".join(bad))


@pytest.mark.parametrize("path", list(kc.PATHS))
def test_knn_magnitudes(path):
    """Scales 1e-30 .. 1e100 on both sets, one huge column, a few huge queries, a few huge reference
    rows in a small and in a large set: fp32 screened distances that underflow, overflow to +inf or
    turn NaN, fp64 distances that are all finite."""
    _run(kc.magnitude_cases(path))


def test_knn_common_offset():
    """X = off + N(0, 1): the error bound's absolute term against the certification gap."""
    _run(kc.offset_cases())


def test_knn_seeded_with_huge_rows():
    """KNN_SEED_MIN_NR rows (pilot, seeds and the seeded screen) with huge queries and rows."""
    _run(kc.seeded_cases())


def test_knn_shape_grid():
    """Nr x Nq around 0, k, the list length, a 16-row step, a tile and a query block, at D = 15, k = 5."""
    _run(kc.grid_cases())


def test_knn_shape_diagonal():
    """Every D x k of the lists with one (Nr, Nq) each, D = 4096, a self window past the end."""
    _run(kc.diagonal_cases())
