"""Edge cases of the exact KNN (csrc/knn*.hip): named, seeded inputs at the magnitudes and sizes
where the fp32 screen, its candidate lists and the certification can go wrong (a plain helper
module like tests/edge_corpus.py: no test, no fixture).

A case's ``data()`` returns ``(ref, labels, query, k, self_offset)``: float64 [Nr, D], int32 [Nr] in
[0, N_CLASSES), float64 [Nq, D].  Every draw is continuous and no row is repeated, so the k + 1
nearest distances of every query are distinct (tests/test_knn_edges_host.py pins that, and that
they are finite, against the C oracle); ties belong to the fallback tests of test_gpu_knn.py.

``fallbacks`` is what the code implies for the number of queries answered by the exhaustive fp64
scan, or None where it implies nothing:
  n           exactly n
  (">=", n)   at least n
 * no split's candidate list can fill (fewer candidates than the list length KC, unit scale): 0.
   A list that is not full leaves the screening cut-off at +inf, which certifies.
 * |q|^2 + max |r|^2 >= 2^125 (the overflow guard): that query falls back; with a reference row
   past fp32's range the max norm is +inf and every query does.
 * squares below fp32's range (scales <= 1e-20): every screened distance is below 1e-38, the bound's
   absolute term is 1e-30, so no cut-off clears it: every query.
 * common offset 1e6: the bound's absolute term ea (|q|^2 + max |r|^2) ~ 4e-6 * 3e13 exceeds every
   screened distance (~ 2 D): every query.

Groups: "magnitude" (per screen path), "offset", "seeded", "grid", "diagonal".
"""
import zlib

import numpy as np

N_CLASSES = 10
SEED_MIN_NR = 32768  # knn.hip KNN_SEED_MIN_NR: the smallest set whose MFMA screen is seeded by a pilot
# one D per screen: MFMA padded to 16, MFMA padded to 32, VALU direct form, chunked direct form
PATHS = {"mfma16": 15, "mfma32": 20, "valu": 16, "hd": 40}
SCALES = (1e-30, 1e-20, 1e-10, 1e6, 1e15, 1e19, 1e20, 1e30, 1e40, 1e100)
HUGE = 1e20          # a component whose square is past fp32 (3.4e38) and far inside fp64
HUGE_QUERIES = (3, 17, 40)
# A query at 1e20 is equally far, in fp64, from every row of a unit-scale set (a row changes its
# distance by 1e-20 of it): a k-fold tie, which these cases must not hold.  So where a few QUERIES
# are huge, both sets are drawn at this scale -- squares ~1e24, well inside fp32, and distances
# from a 1e20 query that differ by ~1e-8 of themselves -- and the huge queries are scaled up from it.
WIDE = 1e12
OFFSETS = (10.0, 30.0, 100.0, 300.0, 1e6)

GRID_D, GRID_K = 15, 5
NQS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)
DS = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49)
KS = (1, 5, 6, 8, 13, 14, 21, 22, 32)


def list_length(D, k):
    """KC, the candidates a screen keeps per query and split (knn.hip knn_layout / pick_kc), for
    sets of at most 32768 rows: k + 3 rounded up to 8 / 16 / 24 / 36, but 6 on the matrix-core
    screen (D < 16 or 16 < D < 32) when k <= 5."""
    if (D < 16 or 16 < D < 32) and k <= 5:
        return 6
    need = k + 3
    return 8 if need <= 8 else 16 if need <= 16 else 24 if need <= 24 else 36


def nr_values(D, k):
    """Reference-set sizes around nothing, k, the list length, one 16-row MFMA step and one tile."""
    kc = list_length(D, k)
    return sorted({0, 1, 2, k - 1, k, k + 1, kc - 1, kc, kc + 1, 15, 16, 17, 255, 256, 257, 513})


class KnnCase:
    def __init__(self, group, name, make, fallbacks=None):
        self.group, self.name, self.fallbacks = group, name, fallbacks
        self._make = make

    def data(self):
        rng = np.random.default_rng(zlib.crc32(("%s/%s" % (self.group, self.name)).encode()))
        ref, query, k, self_offset = self._make(rng)
        labels = rng.integers(0, N_CLASSES, ref.shape[0]).astype(np.int32)
        return np.ascontiguousarray(ref), labels, np.ascontiguousarray(query), k, self_offset

    def __repr__(self):
        return "KnnCase(%s/%s)" % (self.group, self.name)


def _normal(Nr, Nq, D, k, ref_scale=None, query_scale=None, col_scale=None, offset=0.0, base=1.0):
    """ref / query = base * (offset + N(0, 1)), then rows (ref_scale / query_scale: a scalar or
    {row: factor}) and the last column (col_scale) multiplied."""
    def scaled(x, s):
        x *= base
        if isinstance(s, dict):
            for row, f in s.items():
                x[row] *= f
        elif s is not None:
            x *= s
        if col_scale is not None:
            x[:, -1] *= col_scale
        return x

    def make(rng):
        ref = scaled(offset + rng.standard_normal((Nr, D)), ref_scale)
        query = scaled(offset + rng.standard_normal((Nq, D)), query_scale)
        return ref, query, k, -1
    return make


def _shape(Nr, Nq, D, k, self_query):
    """Unit scale; self_query: the first min(Nq, Nr) reference rows ask, each excluded from its own list."""
    def make(rng):
        ref = rng.standard_normal((Nr, D))
        if self_query:
            return ref, ref[:min(Nq, Nr)].copy(), k, 0
        return ref, rng.standard_normal((Nq, D)), k, -1
    return make


def _shape_fallbacks(Nr, D, k, self_query):
    cands = Nr - (1 if self_query and Nr > 0 else 0)
    return 0 if cands < list_length(D, k) else None


def _window(Nr, Nq, D, k):
    """self_offset = Nr - 3: queries 0..2 are the last three reference rows, the rest have no row."""
    def make(rng):
        ref = rng.standard_normal((Nr, D))
        query = rng.standard_normal((Nq, D))
        query[:3] = ref[Nr - 3:]
        return ref, query, k, Nr - 3
    return make


def magnitude_cases(path):
    D, Nr, Nq = PATHS[path], 300, 64
    out = []

    def add(name, make, fallbacks=None):
        out.append(KnnCase("magnitude", "%s/%s" % (path, name), make, fallbacks))

    def uniform_fallbacks(s):
        return Nq if (s <= 1e-20 or s >= 1e19) else None

    for s in SCALES:
        add("uniform_%g" % s, _normal(Nr, Nq, D, 5, ref_scale=s, query_scale=s), uniform_fallbacks(s))
    for s in (1e-20, HUGE):
        add("uniform_%g_k12" % s, _normal(Nr, Nq, D, 12, ref_scale=s, query_scale=s), Nq)
    add("hot_column", _normal(Nr, Nq, D, 5, col_scale=HUGE), Nq)
    add("huge_queries", _normal(Nr, Nq, D, 5, query_scale={r: HUGE / WIDE for r in HUGE_QUERIES}, base=WIDE),
        (">=", len(HUGE_QUERIES)))
    # 3 ordinary rows and 7 far ones: the 5 nearest of every query include 2 far rows
    add("huge_refs_small", _normal(10, Nq, D, 5, ref_scale={r: HUGE for r in (0, 2, 3, 5, 6, 8, 9)}), Nq)
    add("huge_refs_large", _normal(Nr, Nq, D, 5, ref_scale={r: HUGE for r in (1, 16, 63, 64, 130, 255, 256, 299)}), Nq)
    return out


def offset_cases():
    """A common offset makes |q|^2 + max |r|^2 large against the distances: at the middle offsets the
    bound's absolute term is about the gap between the k-th distance and the screening cut-off, the
    one place where a too optimistic error constant gives wrong neighbours instead of a fallback."""
    out = []
    for D in (15, 40):
        for off in OFFSETS:
            out.append(KnnCase("offset", "D%d/off_%g" % (D, off), _normal(3000, 200, D, 5, offset=off),
                               200 if off == 1e6 else None))
    return out


def seeded_cases():
    rows = {r: HUGE / WIDE for r in (0, 5, 4095, 8192, 16384, 20001, 32766, 32767)}
    queries = {q: HUGE / WIDE for q in (0, 7, 15, 16, 31, 32, 48, 63)}
    return [
        KnnCase("seeded", "huge_queries_and_refs",
                _normal(SEED_MIN_NR, 64, 15, 5, ref_scale=rows, query_scale=queries, base=WIDE), 64),
        # the set in range: the other 56 queries go through the pilot, the seeds and the seeded screen
        KnnCase("seeded", "huge_queries", _normal(SEED_MIN_NR, 64, 15, 5, query_scale=queries, base=WIDE),
                (">=", 8)),
    ]


def grid_cases():
    """Every Nr x Nq at (D, k) = (15, 5), as plain queries and as a self-query."""
    out = []
    for Nr in nr_values(GRID_D, GRID_K):
        for Nq in NQS:
            for sq in (False, True):
                out.append(KnnCase("grid", "Nr%d_Nq%d_%s" % (Nr, Nq, "self" if sq else "plain"),
                                   _shape(Nr, Nq, GRID_D, GRID_K, sq), _shape_fallbacks(Nr, GRID_D, GRID_K, sq)))
    return out


def diagonal_cases():
    """Every other (D, k): one Nr and one Nq each, rotating through the lists; the maximum D; a
    self_offset window that runs past the end of the set, on each kind of screen."""
    out, i = [], 0
    for D in DS:
        for k in KS:
            if (D, k) == (GRID_D, GRID_K):
                continue
            nrs = nr_values(D, k)
            Nr, Nq = nrs[i % len(nrs)], NQS[(3 * i + 1) % len(NQS)]
            i += 1
            for sq in (False, True):
                out.append(KnnCase("diagonal", "D%d_k%d_Nr%d_Nq%d_%s" % (D, k, Nr, Nq, "self" if sq else "plain"),
                                   _shape(Nr, Nq, D, k, sq), _shape_fallbacks(Nr, D, k, sq)))
    out.append(KnnCase("diagonal", "D4096", _shape(40, 3, 4096, 3, False)))
    for D in (15, 16, 40):
        out.append(KnnCase("diagonal", "self_window_D%d" % D, _window(300, 10, D, 5)))
    return out


def all_cases():
    out = []
    for path in PATHS:
        out += magnitude_cases(path)
    return out + offset_cases() + seeded_cases() + grid_cases() + diagonal_cases()
