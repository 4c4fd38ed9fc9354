// knn_merge.hip -- the fp64 stages of the exact KNN (pipeline: knn.hip): the re-rank and
// certification of the screened candidates (knn_merge, knn_merge1) and the exhaustive fallback,
// each with its host launcher.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "knn_internal.h"

namespace dsp {

#pragma clang fp contract(off)
// sklearn euclidean_rdist: sequential d += t*t, no FMA
__device__ __forceinline__ double rdist64(const double *__restrict__ a, const double *__restrict__ b, int D)
{
    double d = 0.0;
    for (int c = 0; c < D; c++) {
        const double t = a[c] - b[c];
        d = d + t * t;
    }
    return d;
}
// The same for D <= 16 (the 15-d features) with the query in registers and the reference row's
// loads all issued before its first use: the rolled loop above waited for each of its loads in
// turn, so a re-rank or a fallback scan paid ~D memory latencies per row (round 6: the 3
// fallback queries of the 100k x 100k self-query on extracted features took 1.06 ms).
struct QRow16 {
    double v[16];
};
__device__ __forceinline__ QRow16 qrow16(const double *__restrict__ qx, int D)
{
    QRow16 q;
#pragma unroll
    for (int c = 0; c < 16; c++) q.v[c] = c < D ? qx[c] : 0.0;
    return q;
}
__device__ __forceinline__ void row16_load(double (&b)[16], const double *__restrict__ r, int D)
{
#pragma unroll
    for (int c = 0; c < 16; c++) b[c] = c < D ? r[c] : 0.0;
}
__device__ __forceinline__ double rdist64_16(const QRow16 &q, const double (&b)[16], int D)
{
    double d = 0.0;
#pragma unroll
    for (int c = 0; c < 16; c++)
        if (c < D) {
            const double t = q.v[c] - b[c];
            d = d + t * t;
        }
    return d;
}
// rdist64 through the register path when D <= 16
__device__ __forceinline__ double rdist64_q(const QRow16 &q, const double *__restrict__ qx, const double *__restrict__ r,
                                            int D)
{
    if (D <= 16) {
        double b[16];
        row16_load(b, r, D);
        return rdist64_16(q, b, D);
    }
    return rdist64(qx, r, D);
}
#pragma clang fp contract(on)

__device__ __forceinline__ bool cand_less(double da, int ia, double db, int ib)
{
    return da < db || (da == db && ia < ib);
}

// the KM smallest (distance, index) pairs in ascending order, fixed length (no register array is
// indexed at run time, so the lists stay in registers)
template <int KM>
__device__ __forceinline__ void topk_fixed_insert(double (&dl)[KM], int (&il)[KM], double d, int r)
{
    if (!cand_less(d, r, dl[KM - 1], il[KM - 1])) return;
#pragma unroll
    for (int i = KM - 1; i > 0; i--) {
        const bool shift = cand_less(d, r, dl[i - 1], il[i - 1]);
        const bool here = !shift && cand_less(d, r, dl[i], il[i]);
        dl[i] = shift ? dl[i - 1] : here ? d : dl[i];
        il[i] = shift ? il[i - 1] : here ? r : il[i];
    }
    if (cand_less(d, r, dl[0], il[0])) {
        dl[0] = d;
        il[0] = r;
    }
}
template <int KM, typename T>
__device__ __forceinline__ T kth_of(const T (&a)[KM], int k)  // a[k - 1], k run-time
{
    T v = a[0];
#pragma unroll
    for (int i = 1; i < KM; i++) v = (i == k - 1) ? a[i] : v;
    return v;
}

// ---- what the two merges share: the error bound, pass 1's insert, certification and output ----
// |fp32 screened distance - fp64 distance| <= err(d): fp32 rounding of the inputs and of the sum
// (direct or expanded form), coefficients from the host (knn_err_coeffs)
struct MergeErr {
    double err_rel, err_abs, qn, rmax;
    __device__ __forceinline__ double operator()(double d) const { return err_rel * d + err_abs * (qn + rmax) + 1e-30; }
};
__device__ __forceinline__ MergeErr merge_err(const QRow16 &q16, const double *__restrict__ qx, int D,
                                              const unsigned int *maxnorm_bits, double err_rel, double err_abs)
{
    double qn = 0.0;
    if (D <= 16) {
#pragma unroll
        for (int c = 0; c < 16; c++)
            if (c < D) qn += q16.v[c] * q16.v[c];
    } else {
        for (int c = 0; c < D; c++) qn += qx[c] * qx[c];
    }
    return MergeErr{err_rel, err_abs, qn, (double)__uint_as_float(*maxnorm_bits)};
}
// query q's candidates of split s, loaded together
template <int KC>
__device__ __forceinline__ void load_split(const float *__restrict__ cand_d, const int *__restrict__ cand_i,
                                           int64_t Nq, int64_t q, int s, int (&rr)[KC], float (&dd)[KC])
{
    const size_t o = ((size_t)s * Nq + q) * KC;
#pragma unroll
    for (int i = 0; i < KC; i++) {
        rr[i] = cand_i[o + i];
        dd[i] = cand_d[o + i];
    }
}
// pass 1 (fp32 only) over one split: k32, the KM smallest screened distances so far, its k-th
// (kth), and the screening cut-off of a split whose candidate list is full
template <int KC, int KM>
__device__ __forceinline__ void pass1_insert(const int (&rr)[KC], const float (&dd)[KC], int64_t self, int k,
                                             float (&k32)[KM], float &kth, float &cut)
{
#pragma unroll
    for (int i = 0; i < KC; i++) {
        // a value at or past the k-th so far is not among the k smallest either
        if (rr[i] < 0 || rr[i] == self || !(dd[i] < kth)) continue;
        float v = dd[i];  // sorted insert into the KM smallest
#pragma unroll
        for (int j = 0; j < KM; j++) {
            const float lo = fminf(v, k32[j]);
            v = fmaxf(v, k32[j]);
            k32[j] = lo;
        }
        kth = kth_of<KM>(k32, k);
    }
    if (rr[KC - 1] >= 0) cut = fminf(cut, dd[KC - 1]);
}
// certification: any row that was screened out has fp32 distance >= cut; its true fp64 squared
// distance is >= cut - tol (fp32 rounding of inputs and of the sum).  A query that fails goes on
// the fallback list; one that passes gets its idx / dist and the scipy.stats.mode of the k labels
// (the smallest most frequent).
template <int KM>
__device__ __forceinline__ void certify_and_write(int64_t q, int k, float cut, const MergeErr &err,
                                                  const double (&dl)[KM], const int (&il)[KM],
                                                  const int32_t *__restrict__ labels, int32_t *__restrict__ idx,
                                                  double *__restrict__ dist, int32_t *__restrict__ pred,
                                                  int *fb_count, int *fb_list)
{
    const double tol = err((double)cut);
    // fp32 range first (knn.hip, next to knn_err_coeffs): past it a screened distance may have been
    // +inf or NaN, which no screen keeps and no list counts, so neither "the lists are not full"
    // nor cut says anything about the rows left out.  (A NaN sum fails the compare as well.)
    const bool in_range = err.qn + err.rmax < KNN_F32_SAFE;
    const bool ok = in_range && (!(cut < INFINITY) || ((double)cut - tol > kth_of<KM>(dl, k)));
    if (!ok) {
        const int slot = atomicAdd(fb_count, 1);
        fb_list[slot] = (int)q;
        return;
    }
    int outi[KM];
#pragma unroll
    for (int i = 0; i < KM; i++) {
        const bool valid = dl[i] < INFINITY;
        outi[i] = valid ? il[i] : -1;
        if (i < k) {
            idx[q * k + i] = outi[i];
            dist[q * k + i] = valid ? sqrt(dl[i]) : INFINITY;
        }
    }
    if (pred && labels) {
        int best = -1, bestc = 0;
#pragma unroll
        for (int a = 0; a < KM; a++) {
            if (a >= k || outi[a] < 0) continue;
            const int la = labels[outi[a]];
            int cnt = 0;
#pragma unroll
            for (int b2 = 0; b2 < KM; b2++) cnt += b2 < k && outi[b2] >= 0 && labels[outi[b2]] == la;
            if (cnt > bestc || (cnt == bestc && la < best)) {
                bestc = cnt;
                best = la;
            }
        }
        pred[q] = best;
    }
}

// One thread per query, each split's KC candidates loaded together: lists of KM = 16 / 32 (k > 8;
// the group merge's networks at those lengths cost minutes of compile time per instantiation).
template <int KC, int KM>
__global__ __launch_bounds__(64) void knn_merge1(const double *__restrict__ ref, const double *__restrict__ query,
                          int64_t Nr, int64_t Nq, int D, int k, int nsplit, int64_t self_offset,
                          const float *__restrict__ cand_d, const int *__restrict__ cand_i,
                          const unsigned int *maxnorm_bits, double err_rel, double err_abs,
                          const int32_t *__restrict__ labels, int32_t *__restrict__ idx,
                          double *__restrict__ dist, int32_t *__restrict__ pred, int *fb_count,
                          int *fb_list, const float *__restrict__ seed)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Nq) return;
    const double *qx = query + q * D;
    const QRow16 q16 = qrow16(qx, D <= 16 ? D : 0);
    double dl[KM];
    int il[KM];
    float k32[KM];
#pragma unroll
    for (int i = 0; i < KM; i++) {
        dl[i] = INFINITY;
        il[i] = 0x7fffffff;
        k32[i] = INFINITY;
    }
    const MergeErr err = merge_err(q16, qx, D, maxnorm_bits, err_rel, err_abs);
    const int64_t self = self_offset >= 0 ? self_offset + q : -1;
    // cut: every row the screen did not keep has a screened distance >= cut (a seeded screen keeps
    // only rows below min(seed, the lists' thresholds))
    float kth = INFINITY, cut = seed ? seed[q] : INFINITY;
    for (int s = 0; s < nsplit; s++) {
        int rr[KC];
        float dd[KC];
        load_split<KC>(cand_d, cand_i, Nq, q, s, rr, dd);
        pass1_insert<KC, KM>(rr, dd, self, k, k32, kth, cut);
    }
    // pass 2: fp64 re-rank (sklearn's own distance) of the candidates that can still be among the
    // k nearest: a candidate with d - err(d) > t32 + err(t32) is farther (in fp64) than the k
    // candidates at or below t32
    const double t32 = (double)kth;
    const double keep = t32 < INFINITY ? t32 + err(t32) : INFINITY;
    for (int s = 0; s < nsplit; s++) {
        int rr[KC];
        float dd[KC];
        load_split<KC>(cand_d, cand_i, Nq, q, s, rr, dd);
#pragma unroll
        for (int i = 0; i < KC; i++) {
            const double d = (double)dd[i];
            if (rr[i] < 0 || rr[i] == self || d - err(d) > keep) continue;
            topk_fixed_insert<KM>(dl, il, rdist64_q(q16, qx, ref + (int64_t)rr[i] * D, D), rr[i]);
        }
    }
    certify_and_write<KM>(q, k, cut, err, dl, il, labels, idx, dist, pred, fb_count, fb_list);
}

// the KM smallest of two ascending lists (a: this lane's, the partner's via shuffle) into a,
// ascending: elementwise min of a and the reversed partner list (a bitonic sequence holding the
// KM smallest of the union), then a bitonic merge network
template <int KM>
__device__ __forceinline__ void merge_sorted_f(float (&a)[KM], int m)
{
    float b[KM];
#pragma unroll
    for (int i = 0; i < KM; i++) b[i] = __shfl_xor(a[i], m, 64);
#pragma unroll
    for (int i = 0; i < KM; i++) a[i] = fminf(a[i], b[KM - 1 - i]);
#pragma unroll
    for (int h = KM / 2; h > 0; h >>= 1)
#pragma unroll
        for (int i = 0; i < KM; i++)
            if ((i & h) == 0) {
                const float lo = fminf(a[i], a[i + h]), hi = fmaxf(a[i], a[i + h]);
                a[i] = lo;
                a[i + h] = hi;
            }
}
// the same for (distance, index) pairs in cand_less order (a strict total order: the result is
// the KM smallest pairs of the union whatever the lanes' shares were)
template <int KM>
__device__ __forceinline__ void merge_sorted_pairs(double (&dl)[KM], int (&il)[KM], int m)
{
    double bd[KM];
    int bi[KM];
#pragma unroll
    for (int i = 0; i < KM; i++) {
        bd[i] = __shfl_xor(dl[i], m, 64);
        bi[i] = __shfl_xor(il[i], m, 64);
    }
#pragma unroll
    for (int i = 0; i < KM; i++) {
        const bool t = cand_less(bd[KM - 1 - i], bi[KM - 1 - i], dl[i], il[i]);
        dl[i] = t ? bd[KM - 1 - i] : dl[i];
        il[i] = t ? bi[KM - 1 - i] : il[i];
    }
#pragma unroll
    for (int h = KM / 2; h > 0; h >>= 1)
#pragma unroll
        for (int i = 0; i < KM; i++)
            if ((i & h) == 0) {
                const bool t = cand_less(dl[i + h], il[i + h], dl[i], il[i]);
                const double d0 = dl[i], d1 = dl[i + h];
                const int i0 = il[i], i1 = il[i + h];
                dl[i] = t ? d1 : d0;
                il[i] = t ? i1 : i0;
                dl[i + h] = t ? d0 : d1;
                il[i + h] = t ? i0 : i1;
            }
}

// MG lanes per query (8 queries per wave): lane j of a query's group takes the splits s = j
// (mod MG), keeps its own fp32 k-th list (pass 1) and fp64 (distance, index) list (pass 2), and
// the group merges them by a lane^1 / ^2 / ^4 butterfly.  The k-th smallest of a multiset and
// the KM smallest (distance, index) pairs do not depend on how the candidates were shared, so
// the results equal one thread walking every split (round 3's knn_merge); with MG times the
// threads, a 12 500-query shard fills the chip instead of 196 waves.
template <int KC, int KM>
__global__ __launch_bounds__(64) void knn_merge(const double *__restrict__ ref, const double *__restrict__ query,
                          int64_t Nr, int64_t Nq, int D, int k, int nsplit, int64_t self_offset,
                          const float *__restrict__ cand_d, const int *__restrict__ cand_i,
                          const unsigned int *maxnorm_bits, double err_rel, double err_abs,
                          const int32_t *__restrict__ labels, int32_t *__restrict__ idx,
                          double *__restrict__ dist, int32_t *__restrict__ pred, int *fb_count,
                          int *fb_list, const float *__restrict__ seed)
{
    const int j = threadIdx.x % MG;
    const int64_t qr = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / MG;
    const bool live = qr < Nq;  // every lane takes part in the shuffles
    const int64_t q = live ? qr : Nq - 1;
    const double *qx = query + q * D;
    const QRow16 q16 = qrow16(qx, D <= 16 ? D : 0);
    double dl[KM];
    int il[KM];
    float k32[KM];
#pragma unroll
    for (int i = 0; i < KM; i++) {
        dl[i] = INFINITY;
        il[i] = 0x7fffffff;
        k32[i] = INFINITY;
    }
    const MergeErr err = merge_err(q16, qx, D, maxnorm_bits, err_rel, err_abs);
    const int64_t self = self_offset >= 0 ? self_offset + q : -1;
    // cut: every row the screen did not keep has a screened distance >= cut (a seeded screen keeps
    // only rows below min(seed, the lists' thresholds))
    float kth = INFINITY, cut = seed ? seed[q] : INFINITY;
    // pass 1 over this lane's splits (a value at or past the lane's k-th is not among the group's
    // k smallest either)
    auto load = [&](int s, int (&rr)[KC], float (&dd)[KC]) { load_split<KC>(cand_d, cand_i, Nq, q, s, rr, dd); };
    auto pass1 = [&](const int (&rr)[KC], const float (&dd)[KC]) { pass1_insert<KC, KM>(rr, dd, self, k, k32, kth, cut); };
    // short lists (KC <= 8): a lane's first two splits are loaded together and kept in registers
    // for pass 2 (12 500 queries take 13 splits, 100 000 take 6: every split of MG = 8 lanes)
    constexpr bool CACHE2 = KC <= 8;
    constexpr int NC = CACHE2 ? KC : 1;
    int rc0[NC], rc1[NC];
    float dc0[NC], dc1[NC];
    const bool h0 = CACHE2 && j < nsplit, h1 = CACHE2 && j + MG < nsplit;
    if constexpr (CACHE2) {
        if (h0) load(j, rc0, dc0);
        if (h1) load(j + MG, rc1, dc1);
        if (h0) pass1(rc0, dc0);
        if (h1) pass1(rc1, dc1);
    }
    for (int s = j + (CACHE2 ? 2 * MG : 0); s < nsplit; s += MG) {
        int rr[KC];
        float dd[KC];
        load(s, rr, dd);
        pass1(rr, dd);
    }
#pragma unroll
    for (int m = 1; m < MG; m <<= 1) {
        merge_sorted_f<KM>(k32, m);
        cut = fminf(cut, __shfl_xor(cut, m, 64));
    }
    kth = kth_of<KM>(k32, k);
    // pass 2: fp64 re-rank (sklearn's own distance) of the candidates that can still be among the
    // k nearest: a candidate with d - err(d) > t32 + err(t32) is farther (in fp64) than the k
    // candidates at or below t32
    const double t32 = (double)kth;
    const double keep = t32 < INFINITY ? t32 + err(t32) : INFINITY;
    // the candidates that pass are few (about k per query over its MG lanes): a bit mask, then ONE
    // rolled loop that picks each candidate by selects -- unrolling the row loads, the distance and
    // the list insert per candidate slot made this kernel ~15k instructions (instruction-cache
    // misses) for no gain
    auto need = [&](int r, float df) {
        const double d = (double)df;
        return !(r < 0 || r == self || d - err(d) > keep);
    };
    auto rerank = [&](int r) { topk_fixed_insert<KM>(dl, il, rdist64_q(q16, qx, ref + (int64_t)r * D, D), r); };
    if constexpr (CACHE2) {
        unsigned mask = 0;
#pragma unroll
        for (int i = 0; i < KC; i++) {
            if (h0 && need(rc0[i], dc0[i])) mask |= 1u << i;
            if (h1 && need(rc1[i], dc1[i])) mask |= 1u << (KC + i);
        }
        while (mask) {
            const int bit = __builtin_ctz(mask);
            mask &= mask - 1;
            int r = rc0[0];
#pragma unroll
            for (int i = 0; i < KC; i++) {
                r = bit == i ? rc0[i] : r;
                r = bit == KC + i ? rc1[i] : r;
            }
            rerank(r);
        }
    }
    for (int s = j + (CACHE2 ? 2 * MG : 0); s < nsplit; s += MG) {
        int rr[KC];
        float dd[KC];
        load(s, rr, dd);
        unsigned long long mask = 0;
#pragma unroll
        for (int i = 0; i < KC; i++)
            if (need(rr[i], dd[i])) mask |= 1ull << i;
        while (mask) {
            const int bit = __builtin_ctzll(mask);
            mask &= mask - 1;
            int r = rr[0];
#pragma unroll
            for (int i = 1; i < KC; i++) r = bit == i ? rr[i] : r;
            rerank(r);
        }
    }
#pragma unroll
    for (int m = 1; m < MG; m <<= 1) merge_sorted_pairs<KM>(dl, il, m);
    if (!live || j != 0) return;
    certify_and_write<KM>(q, k, cut, err, dl, il, labels, idx, dist, pred, fb_count, fb_list);
}

// exhaustive fp64 for the queries the screen could not certify (fb_list[0 .. cnt)), in cand_less
// order like every other stage.  Two roles in one launch (no host round trip to learn cnt):
//  * blocks [0, nbp): the first FB_C listed queries, each query's reference rows cut into P parts
//    of prow rows, ONE WAVE per part: every lane keeps the KM smallest of its rows in registers,
//    the wave takes the part's k smallest by k rounds of a butterfly minimum (the winning lane
//    pops its head), writes them to the workspace, and the wave that finishes a query's last part
//    (a per-query counter, zeroed with the fallback count) merges the P lists the same way, one
//    lane per part.  Round 5 scanned a query with one workgroup: the 3 fallback queries of the
//    100k x 100k self-query on extracted features took 0.71-1.06 ms on 3 CUs.
//  * blocks [nbp, grid): the listed queries past FB_C (only when a launch has that many), one
//    workgroup per query: per-thread lists, then a tree merge through LDS.

// the smallest (d, i) over the wave in cand_less order, on every lane
__device__ __forceinline__ void wave_min_pair(double &d, int &i)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double od = __shfl_xor(d, m, 64);
        const int oi = __shfl_xor(i, m, 64);
        if (cand_less(od, oi, d, i)) {
            d = od;
            i = oi;
        }
    }
}
// k rounds: the wave's k smallest of the lanes' ascending KM-lists (consumed); lane j < k returns
// the j-th in (od, oi)
template <int KM>
__device__ __forceinline__ void wave_take_k(double (&dl)[KM], int (&il)[KM], int k, int lane, double &od, int &oi)
{
    od = INFINITY;
    oi = 0x7fffffff;
    for (int j = 0; j < k; j++) {
        double d = dl[0];
        int i = il[0];
        wave_min_pair(d, i);
        if (lane == j) {
            od = d;
            oi = i;
        }
        if (dl[0] == d && il[0] == i && d < INFINITY) {  // this lane's head won: pop it
#pragma unroll
            for (int t = 0; t < KM - 1; t++) {
                dl[t] = dl[t + 1];
                il[t] = il[t + 1];
            }
            dl[KM - 1] = INFINITY;
            il[KM - 1] = 0x7fffffff;
        }
    }
}
// idx / dist / pred of query q from the k results held by lanes 0 .. k-1
template <int KM>
__device__ __forceinline__ void fb_write(int64_t q, int k, int lane, double od, int oi, const int32_t *labels,
                                         int32_t *idx, double *dist, int32_t *pred)
{
    const bool valid = od < INFINITY;
    if (lane < k) {
        idx[q * k + lane] = valid ? oi : -1;
        dist[q * k + lane] = valid ? sqrt(od) : INFINITY;
    }
    if (pred && labels) {
        const int lab = (lane < k && valid) ? labels[oi] : -1;
        int best = -1, bestc = 0;
#pragma unroll
        for (int a = 0; a < KM; a++) {
            if (a >= k) break;
            const int la = __shfl(lab, a, 64);
            if (la < 0) continue;
            int cnt = 0;
#pragma unroll
            for (int b2 = 0; b2 < KM; b2++)
                if (b2 < k) cnt += __shfl(lab, b2, 64) == la;
            if (cnt > bestc || (cnt == bestc && la < best)) {
                bestc = cnt;
                best = la;
            }
        }
        if (lane == 0) pred[q] = best;
    }
}

template <int KM>
__global__ __launch_bounds__(FB_T) void knn_fallback(const double *__restrict__ ref,
                                                     const double *__restrict__ query, int64_t Nr,
                                                     int D, int k, int64_t self_offset,
                                                     const int *fb_count, const int *fb_list,
                                                     const int32_t *__restrict__ labels,
                                                     int32_t *__restrict__ idx,
                                                     double *__restrict__ dist,
                                                     int32_t *__restrict__ pred, int P, int64_t prow, int nbp,
                                                     double *part_d, int *part_i, int *part_done)
{
    const int cnt = *fb_count;
    const int tid = threadIdx.x, lane = tid & 63;
    if ((int)blockIdx.x < nbp) {  // ---- partitioned scan of the first FB_C listed queries
        const int ncnt = min(cnt, FB_C);
        const int nw = nbp * (FB_T / 64);
        for (int u = (int)blockIdx.x * (FB_T / 64) + (tid >> 6); u < ncnt * P; u += nw) {
            const int item = u / P, part = u - item * P;
            const int64_t q = fb_list[item];
            const double *qx = query + q * D;
            const int64_t self = self_offset >= 0 ? self_offset + q : -1;
            const int64_t r0 = (int64_t)part * prow, r1 = min(Nr, r0 + prow);
            double dl[KM];
            int il[KM];
#pragma unroll
            for (int i = 0; i < KM; i++) {
                dl[i] = INFINITY;
                il[i] = 0x7fffffff;
            }
            if (D <= 16) {  // two rows in flight per lane, the query in registers (four: 55.7 against
                            // 46.6 us for the 3 fallbacks of the 100k self-query)
                const QRow16 q16 = qrow16(qx, D);
                for (int64_t r = r0 + lane; r < r1; r += 128) {
                    double b[2][16];
                    row16_load(b[0], ref + r * D, D);
                    row16_load(b[1], ref + (r + 64 < r1 ? r + 64 : r) * D, D);
                    if (r != self) topk_fixed_insert<KM>(dl, il, rdist64_16(q16, b[0], D), (int)r);
                    if (r + 64 < r1 && r + 64 != self) topk_fixed_insert<KM>(dl, il, rdist64_16(q16, b[1], D), (int)(r + 64));
                }
            } else {
                for (int64_t r = r0 + lane; r < r1; r += 64)
                    if (r != self) topk_fixed_insert<KM>(dl, il, rdist64(qx, ref + r * D, D), (int)r);
            }
            double od;
            int oi;
            wave_take_k<KM>(dl, il, k, lane, od, oi);
            const int64_t o = ((int64_t)item * P + part) * KM;
            if (lane < k) {
                part_d[o + lane] = od;
                part_i[o + lane] = oi;
            }
            __threadfence();  // the part's list is visible device-wide (all XCDs) before it is counted
            int last = 0;
            if (lane == 0) last = atomicAdd(&part_done[item], 1) == P - 1;
            if (!__shfl(last, 0, 64)) continue;
            __threadfence();  // acquire: every part's list, from whichever XCD wrote it
            // the final merge: lane p holds part p's ascending list
#pragma unroll
            for (int i = 0; i < KM; i++) {
                const bool in = lane < P && i < k;
                dl[i] = in ? part_d[((int64_t)item * P + lane) * KM + i] : INFINITY;
                il[i] = in ? part_i[((int64_t)item * P + lane) * KM + i] : 0x7fffffff;
            }
            wave_take_k<KM>(dl, il, k, lane, od, oi);
            fb_write<KM>(q, k, lane, od, oi, labels, idx, dist, pred);
        }
        return;
    }
    // ---- one workgroup per listed query past FB_C
    __shared__ double sd[FB_T / 2 * KM];
    __shared__ int si[FB_T / 2 * KM];
    const int nbo = (int)gridDim.x - nbp;
    for (int item = FB_C + (int)blockIdx.x - nbp; item < cnt; item += nbo) {
        const int64_t q = fb_list[item];
        const double *qx = query + q * D;
        const int64_t self = self_offset >= 0 ? self_offset + q : -1;
        double dl[KM];
        int il[KM];
#pragma unroll
        for (int i = 0; i < KM; i++) {
            dl[i] = INFINITY;
            il[i] = 0x7fffffff;
        }
        if (D <= 16) {
            const QRow16 q16 = qrow16(qx, D);
            for (int64_t r = tid; r < Nr; r += FB_T) {
                double b[16];
                row16_load(b, ref + r * D, D);
                if (r != self) topk_fixed_insert<KM>(dl, il, rdist64_16(q16, b, D), (int)r);
            }
        } else {
            for (int64_t r = tid; r < Nr; r += FB_T)
                if (r != self) topk_fixed_insert<KM>(dl, il, rdist64(qx, ref + r * D, D), (int)r);
        }
        // pairwise tree merge of the per-thread lists through LDS
        for (int width = FB_T; width > 1; width >>= 1) {
            const int half = width >> 1;
            __syncthreads();
            if (tid >= half && tid < width)
#pragma unroll
                for (int i = 0; i < KM; i++) {
                    sd[(tid - half) * KM + i] = dl[i];
                    si[(tid - half) * KM + i] = il[i];
                }
            __syncthreads();
            if (tid < half)
#pragma unroll
                for (int i = 0; i < KM; i++)
                    if (i < k) topk_fixed_insert<KM>(dl, il, sd[tid * KM + i], si[tid * KM + i]);
        }
        if (tid < 64) {  // wave 0: thread 0 holds the k smallest; spread them over lanes 0 .. k-1
            double od = INFINITY;
            int oi = 0x7fffffff;
#pragma unroll
            for (int i = 0; i < KM; i++) {
                const double d = __shfl(dl[i], 0, 64);
                const int ii = __shfl(il[i], 0, 64);
                if (lane == i) {
                    od = d;
                    oi = ii;
                }
            }
            fb_write<KM>(q, k, lane, od, oi, labels, idx, dist, pred);
        }
        __syncthreads();
    }
}

// ---- host launchers (knn_internal.h) ----
bool launch_knn_merge(hipStream_t s, int KC, const double *ref, const double *query, int64_t Nr, int64_t Nq, int D,
                      int k, int nsplit, int64_t self_offset, const float *cand_d, const int *cand_i,
                      const unsigned int *maxnorm_bits, double err_rel, double err_abs, const int32_t *labels,
                      int32_t *idx, double *dist, int32_t *pred, int *fb_count, int *fb_list, const float *seed)
{
    // 64-thread workgroups.  knn_merge (k <= 8), MG lanes per query: 12 500 queries (one rank of the
    // 8-GPU self-query) are 1 563 of them; knn_merge1 (k > 8), one thread per query
    const dim3 g((unsigned)((Nq * MG + 63) / 64)), g1((unsigned)((Nq + 63) / 64)), b(64);
    bool merged = false;
    dispatch_kc(KC, [&](auto kc) {
        constexpr int C = kc();
        auto go = [&](auto kernel, dim3 grid) {
            hipLaunchKernelGGL(kernel, grid, b, 0, s, ref, query, Nr, Nq, D, k, nsplit, self_offset, cand_d, cand_i,
                               maxnorm_bits, err_rel, err_abs, labels, idx, dist, pred, fb_count, fb_list, seed);
            merged = true;
        };
        // KC >= k + KNN_SLACK, so KC = 8 implies k <= 8 and KC = 16 implies k <= 16
        if (k > C) return;
        if (k <= 8) return go(knn_merge<C, 8>, g);
        if constexpr (C >= 16)
            if (k <= 16) return go(knn_merge1<C, 16>, g1);
        if constexpr (C >= 24) go(knn_merge1<C, 32>, g1);
    });
    return merged;
}

void launch_knn_fallback(hipStream_t s, int KM, const double *ref, const double *query, int64_t Nr, int64_t Nq, int D,
                         int k, int64_t self_offset, const int *fb_count, const int *fb_list, const int32_t *labels,
                         int32_t *idx, double *dist, int32_t *pred, int P, double *part_d, int *part_i,
                         int *part_done)
{
    // partitioned role: enough waves for every part of FB_C queries, at most 1 024 (most launches
    // list no query and these workgroups return at once); the per-workgroup role only when this
    // launch can list more than FB_C queries
    const int64_t prow = (Nr + P - 1) / P;
    const int nbp = (int)std::min<int64_t>(256, ((int64_t)std::min<int64_t>(Nq, FB_C) * P + 3) / 4);
    const int nbo = Nq > FB_C ? (int)std::min<int64_t>(512, Nq - FB_C) : 0;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)(nbp + nbo)), dim3(FB_T), 0, s, ref, query, Nr, D, k, self_offset,
                           fb_count, fb_list, labels, idx, dist, pred, P, prow, nbp, part_d, part_i, part_done);
    };
    if (KM == 8) go(knn_fallback<8>); else if (KM == 16) go(knn_fallback<16>); else go(knn_fallback<32>);
}

}  // namespace dsp
