"""CPU checks behind the KNN and z-score edge tests: the KNN edge cases (tests/knn_edge_cases.py)
are inside the contract and tie-free under the C oracle, and the oracle's z-score is numpy's own
np.mean / np.std over axis 0, bit for bit, one column included."""
import numpy as np
import pytest

import knn_edge_cases as kc
import oracle
import zscore_edge_cases as zc


def test_case_names_are_unique_and_cover_the_groups():
    cases = kc.all_cases()
    names = [(c.group, c.name) for c in cases]
    assert len(set(names)) == len(names)
    assert {c.group for c in cases} == {"magnitude", "offset", "seeded", "grid", "diagonal"}
    # deterministic: a second build of a case gives the same arrays
    c = kc.magnitude_cases("mfma16")[0]
    assert all(np.array_equal(a, b) for a, b in zip(c.data()[:3], c.data()[:3]))


def test_list_length_brackets_k():
    for D in kc.DS:
        for k in kc.KS:
            KC = kc.list_length(D, k)
            assert KC > k and {k - 1, k, k + 1, KC - 1, KC, KC + 1, 0, 16, 257} <= set(kc.nr_values(D, k))


def _assert_fair(case):
    """The oracle's k + 1 nearest: finite, strictly increasing distances wherever there is a row, so
    the k nearest are unique (no tie at the k-th either) and every distance is inside fp64."""
    ref, labels, query, k, self_offset = case.data()
    assert ref.dtype == np.float64 and query.dtype == np.float64 and labels.dtype == np.int32
    assert np.isfinite(ref).all() and np.isfinite(query).all(), case
    assert labels.shape == (ref.shape[0],) and ref.shape[1] == query.shape[1]
    idx, dist, _ = oracle.knn(ref, labels, query, k + 1, n_classes=kc.N_CLASSES, self_offset=self_offset,
                              nthreads=8)
    have = idx >= 0
    cands = ref.shape[0] - (self_offset >= 0) * ((self_offset + np.arange(query.shape[0])) < ref.shape[0])
    assert np.array_equal(have.sum(1), np.minimum(cands, k + 1)), case
    assert np.isfinite(dist[have]).all(), case
    assert np.isinf(dist[~have]).all(), case
    both = have[:, 1:]
    assert (dist[:, 1:][both] > dist[:, :-1][both]).all(), case
    return have


@pytest.mark.parametrize("path", list(kc.PATHS))
def test_magnitude_cases_are_fair(path):
    cases = kc.magnitude_cases(path)
    assert len(cases) == len(kc.SCALES) + 6
    for c in cases:
        have = _assert_fair(c)
        assert have.all(), c
    # the small set: 3 ordinary rows, so 2 of every query's 5 nearest are rows at 1e20
    ref, labels, query, k, so = [c for c in cases if c.name.endswith("huge_refs_small")][0].data()
    _, dist, _ = oracle.knn(ref, labels, query, k, n_classes=kc.N_CLASSES)
    assert ((dist > 1e15).sum(1) == 2).all()


def test_offset_and_seeded_cases_are_fair():
    for c in kc.offset_cases() + kc.seeded_cases():
        assert _assert_fair(c).all(), c
    assert kc.seeded_cases()[0].data()[0].shape[0] == kc.SEED_MIN_NR


def test_shape_cases_are_fair():
    grid, diag = kc.grid_cases(), kc.diagonal_cases()
    assert len(grid) == 2 * len(kc.nr_values(kc.GRID_D, kc.GRID_K)) * len(kc.NQS)
    assert len(diag) == 2 * (len(kc.DS) * len(kc.KS) - 1) + 4
    short = 0
    for c in grid + diag:
        have = _assert_fair(c)
        short += int(have.size > 0 and not have[:, :-1].all())
        if c.fallbacks == 0:  # fewer candidates than a list holds
            assert not have.size or have.sum(1).max() < kc.list_length(c.data()[0].shape[1], c.data()[3]), c
    assert short > 40  # cases with fewer than k candidates exist in number


def test_workspace_bytes_of_an_empty_query_batch():
    """dsp_knn_workspace_bytes is host code (no GPU): Nq = 0 is a size like any other, on every
    screen's layout and on the seeded one (it divided by the number of query blocks)."""
    from src import _hip
    L = _hip.lib()
    for D in kc.DS + (40, 4096):
        for Nr in (0, 1, 300, kc.SEED_MIN_NR, 100000):
            for k in (1, 5, 32):
                b0 = L.dsp_knn_workspace_bytes(Nr, 0, D, k)
                assert 0 < b0 <= L.dsp_knn_workspace_bytes(Nr, 1, D, k), (Nr, D, k)
                assert L.dsp_knn_workspace_fallbacks_offset(Nr, 0, D, k) < b0


# ---- the oracle's z-score is numpy's ----

def _numpy_fit(X):
    mean, std = np.mean(X, axis=0), np.std(X, axis=0)
    return mean, np.where(std == 0, 1.0, std)


def _oracle_fit(X):
    mean, std = oracle.zscore_fit(X)
    return mean, np.where(std == 0, 1.0, std)


def test_oracle_zscore_is_numpy():
    for name, X in zc.matrices():
        assert X.flags.c_contiguous and X.dtype == np.float64
        m0, s0 = _numpy_fit(X)
        m1, s1 = _oracle_fit(X)
        assert np.array_equal(m1, m0), name
        assert np.array_equal(s1, s0), name


def test_oracle_zscore_one_column_long():
    """Every branch of the pairwise rule and deep recursion: lengths around 8, 128 and the splits."""
    rng = np.random.default_rng(5)
    for N in list(range(1, 300)) + [511, 512, 513, 1023, 1024, 1025, 4097, 8191, 8192, 8193, 16385, 100000]:
        X = (37.0 + 3.0 * rng.standard_normal((N, 1)))
        m0, s0 = _numpy_fit(X)
        m1, s1 = _oracle_fit(X)
        assert np.array_equal(m1, m0) and np.array_equal(s1, s0), N
