// knn.hip -- exact k-nearest-neighbour classification for gfx950 (CDNA4).
//
// Replaces KNeighborsClassifier(n_neighbors=k).fit/predict/kneighbors as used by
// src/models.py:33-35,52-58 (sklearn 1.7.2: algorithm='auto' -> kd_tree, minkowski p=2,
// uniform weights, scipy.stats.mode vote).
//
// Pipeline (all stream-ordered, no host sync):
//   1. knn_convert      fp64 [N,D] -> fp32 [N,DP] zero-padded rows (+ max row norm^2, for the
//                       bound); D < DP: expanded form, references (-2 r, |r|^2), queries (q, 1)
//   2. screen           grid (query block, reference split); each query keeps the KC smallest
//                       fp32 squared distances (KC = k + 3 slack, rounded up) of its split; the
//                       [Nq x Nr] distance matrix is never materialised:
//        knn_screen_mfma  D < DP (the 15-d features): |q|^2 + q'.r' on v_mfma_f32_16x16x4_f32
//        knn_screen       D = 16 or 32: direct form (q - r)^2 on the VALU
//        knn_screen_hd    D > 32 (flattened sequences): direct form in chunks of 16 dimensions
//   3. knn_merge        one thread per query: re-ranks every surviving candidate with the
//                       reference's own fp64 distance (sequential sum of squared differences, no
//                       FMA -- sklearn euclidean_rdist), keeps the k best by (distance, index), and
//                       certifies that no screened-out row can beat the k-th; otherwise the query
//                       goes on a fallback list.
//   4. knn_fallback     exhaustive fp64 scan of the listed queries: each query's rows in parts,
//                       one wave per part, the parts' lists merged by the last wave done.
//   5. vote             majority label, smallest label on ties (scipy.stats.mode).
//
// This file is the host side: the workspace layout, the launch shapes and the C entry points.
// Stages 1-2 are in knn_screen.hip, 3-5 in knn_merge.hip; knn_internal.h holds what they share.
// DSP_KNN_DIAG (the knndiag library) changes host code here only, so that library links the
// product's own device objects.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "dsp_audiorec.h"
#include "knn_internal.h"

namespace {
struct KnnLayout {
    size_t ref32, refmx, q32, cand_d, cand_i, misc, fb_d, fb_i, pilot_d, seed, total;
    int fb_parts, fb_km;  // partitioned fallback: parts per query, list length
    int DP, KC, nsplit;
    int rstride, nsample, nsplit_p;  // seeded thresholds (rstride > 0): sample rows j * rstride
    bool exp;  // expanded-form screening (a spare padded column holds |r|^2)
    bool hd;   // D > 32: chunked direct-form screen (knn_screen_hd)
    bool mfma; // expanded form on the matrix cores (knn_screen_mfma)
};

static constexpr int KNN_DMAX = 4096;
// seeded thresholds: a pilot over ~KNN_SEED_SAMPLE strided rows when the set has >= KNN_SEED_MIN_NR.
// Round 5: the pilot keeps class minima (knn_pilot_mfma) instead of top-KC lists -- at 4 096 rows
// 84.8 -> 31.5 us at 12.5k queries, 409 -> 197 us at 100k, whole job 0.795-0.807 -> 0.738-0.757 ms
// and 4.46-4.54 -> 4.27 ms (profiles/r05k2_knn_ab.txt) -- and the cheaper pilot affords a larger
// sample: 2 048 / 4 096 / 8 192 / 16 384 rows 0.81-0.83 / 0.76 / 0.716-0.721 / 0.73-0.74 ms at 12.5k,
// 4.45-4.48 / 4.27-4.30 / 4.15-4.20 / 4.30-4.34 ms at 100k (profiles/r05k2_pilot_sweep.txt).
// The pilot of top-KC lists, with or without a pre-pilot of its own, is removed; its record is
// profiles/r05k2_* and profiles/r05_knn_pilot_sweep.txt.
#ifndef KNN_SEED_SAMPLE
#define KNN_SEED_SAMPLE 8192
#endif
#ifndef KNN_SEED_MIN_NR
#define KNN_SEED_MIN_NR 32768
#endif
#ifndef KNN_SEED_WARM
#define KNN_SEED_WARM 1024.0
#endif
#ifndef KNN_SEED_SAT
#define KNN_SEED_SAT 16
#endif

int pick_kc(int k)
{
    const int need = k + dsp::KNN_SLACK;
    if (need <= 8) return 8;
    if (need <= 16) return 16;
    if (need <= 24) return 24;
    return 36;
}

// MFMA screen: reference splits.  Every workgroup of the grid is resident at once, so a CU's time
// is (rows per split + a split's list warm-up W) x its waves, and a CU saturates at `sat` waves:
// T(s) = (Nr / s + W) * max(waves on the busiest CU, sat).  From a threshold at +inf, W ~ 16k rows
// and two waves per SIMD saturate (sat 8); from a seeded threshold W ~ 1k rows, and a step then
// inserts so rarely that the steps' dependency chains need four waves per SIMD to hide (sat 16):
// 12.5k x 100k forced splits 4 / 6 / 8 / 10 / 12 / 16 / 20 measured 1.08 / 1.00 / 0.97 / 0.86 /
// 0.87 / 0.91 / 0.88 ms (profiles/r04_knn_split_sweep.txt).
int pick_nsplit_mfma(int64_t Nr, int64_t Nq, int qpb, int cus, double warm = 16384.0, int sat = 8)
{
    const int64_t qblocks = (Nq + qpb - 1) / qpb;
    const int64_t maxs = std::max<int64_t>(1, std::min<int64_t>(64, (Nr + dsp::MQ_TR - 1) / dsp::MQ_TR));
    int best = 1;
    double best_t = 1e300;
    for (int64_t s = 1; s <= maxs; s++) {
        const int64_t waves = (qblocks * s + cus - 1) / cus * dsp::MQ_W;
        const double t = ((double)Nr / (double)s + warm) * (double)std::max<int64_t>(waves, sat);
        if (t < best_t * (1.0 - 1e-9)) {
            best_t = t;
            best = (int)s;
        }
    }
    return best;
}

int pick_nsplit(int64_t Nr, int64_t Nq, int qpb)
{
    // (an empty query batch is sized like one block: dsp_knn_workspace_bytes takes Nq = 0)
    const int64_t qblocks = std::max<int64_t>(1, (Nq + qpb - 1) / qpb);
    // Enough workgroups to fill the chip (two per CU), as few reference splits as that allows:
    // a longer split makes a screened distance that enters its top list rarer (~KC / rows seen),
    // and a wave pays for an insertion whenever any of its 64 lanes makes one
#ifdef DSP_KNN_DIAG  // diagnostic build only (tools/knn_split_sweep.sh): launch-shape override
    static const int target = [] {
        const char *e = getenv("DSP_KNN_TARGET_WGS");
        return e ? atoi(e) : 512;
    }();
#else
    constexpr int target = 512;
#endif
    int64_t s = (target + qblocks - 1) / qblocks;
    const int64_t maxs = (Nr + dsp::KNN_TR - 1) / dsp::KNN_TR;  // >= one tile per split
    if (s > maxs) s = maxs;
    if (s > 64) s = 64;
    if (s < 1) s = 1;
    return (int)s;
}

size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// CUs of the current device, cached
int device_cus()
{
    static int cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cache[dev] == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
        cache[dev] = cus;
    }
    return cache[dev];
}

KnnLayout knn_layout(int64_t Nr, int64_t Nq, int D, int k)
{
    KnnLayout l;
    l.hd = D > 32;
    l.DP = D <= 16 ? 16 : D <= 32 ? 32 : (D + 15) & ~15;
    l.exp = !l.hd && D < l.DP;
    l.KC = pick_kc(k);
    l.mfma = l.exp;  // every expanded-form screen runs on the matrix cores

    // seeded thresholds (matrix-core screen, reference sets of >= KNN_SEED_MIN_NR rows): a pilot
    // screen over every rstride-th row (~KNN_SEED_SAMPLE rows) seeds each query's threshold
    l.rstride = l.nsample = l.nsplit_p = 0;
    if (l.mfma && Nr >= KNN_SEED_MIN_NR) {
        int64_t samp = KNN_SEED_SAMPLE;
#ifdef DSP_KNN_DIAG  // diagnostic build only: pilot sample size
        if (const char *e = getenv("DSP_KNN_SAMPLE")) samp = std::max(64, atoi(e));
#endif
        l.rstride = (int)std::max<int64_t>(2, Nr / samp);
        l.nsample = (int)((Nr + l.rstride - 1) / l.rstride);
    }
#ifdef DSP_KNN_DIAG  // diagnostic build only: seeding off (DSP_KNN_SEED=0)
    if (const char *e = getenv("DSP_KNN_SEED"))
        if (atoi(e) == 0) l.rstride = l.nsample = 0;
#endif
    l.nsplit = l.mfma ? pick_nsplit_mfma(Nr, Nq, dsp::mq_qpb(l.KC), device_cus(),
                                         l.rstride ? KNN_SEED_WARM : 16384.0, l.rstride ? KNN_SEED_SAT : 8)
                      : pick_nsplit(Nr, Nq, l.hd ? dsp::KNN_TQ : dsp::KNN_TQ * dsp::KNN_QP);
#ifdef DSP_KNN_DIAG  // diagnostic build only: forced split count (tools/knn_split_sweep.sh)
    if (const char *e = getenv("DSP_KNN_NSPLIT")) l.nsplit = std::max(1, std::min(64, atoi(e)));
#endif
    // matrix-core screen over short splits (<= 32k rows), k <= 5: six candidates per split
    // (slack 1 instead of 3).  A short split's cost is mostly its list warm-up, and a shorter list
    // inserts less often and more cheaply (12.5k x 100k, 5 splits of 20k rows: 1.19 -> 1.05 ms);
    // over long splits the longer list measured faster (100k x 100k, 2 splits of 50k rows: 5.58
    // against 6.06 ms) and stays.  Same tiles per wave (mq_tiles): the split count is unchanged.
    if (l.mfma && k <= 5 && (Nr + l.nsplit - 1) / l.nsplit <= 32768) l.KC = 6;
    size_t o = 0;
    // the converted reference set and its max row norm first, at offsets that depend on (Nr, D)
    // only: a workspace reused for the same reference set keeps them (DSP_KNN_REF_READY)
    l.ref32 = o; o += al((size_t)Nr * l.DP * 4);
    l.refmx = o; o += al(4);
    l.q32 = o;   o += al((size_t)Nq * l.DP * 4);
    l.cand_d = o; o += al((size_t)l.nsplit * Nq * l.KC * 4);
    l.cand_i = o; o += al((size_t)l.nsplit * Nq * l.KC * 4);
    // (unused), fallback count, 2 words (unused), the per-query part counters of the partitioned
    // fallback (FB_C words, zeroed with the count), the fallback list
    l.misc = o;  o += al(16 + 4 * (size_t)dsp::FB_C + (size_t)Nq * 4);
    l.fb_parts = (int)std::max<int64_t>(1, std::min<int64_t>(dsp::FB_PMAX, (Nr + dsp::FB_PROWS - 1) / dsp::FB_PROWS));
    l.fb_km = k <= 8 ? 8 : k <= 16 ? 16 : 32;
    {
        const size_t nfb = (size_t)std::min<int64_t>(Nq, dsp::FB_C) * l.fb_parts * l.fb_km;
        l.fb_d = o; o += al(nfb * 8);
        l.fb_i = o; o += al(nfb * 4);
    }
    l.pilot_d = l.seed = 0;
    if (l.rstride) {
        // pilot splits: enough workgroups to fill the chip twice over, >= one tile of rows each
        const int64_t qblocks = std::max<int64_t>(1, (Nq + dsp::mq_qpb(l.KC) - 1) / dsp::mq_qpb(l.KC));
        l.nsplit_p = (int)std::max<int64_t>(1, std::min<int64_t>({(2 * device_cus() + qblocks - 1) / qblocks,
                                                                  (l.nsample + dsp::MQ_TR - 1) / dsp::MQ_TR, 64}));
        l.pilot_d = o; o += al((size_t)l.nsplit_p * Nq * dsp::PIL_CLS * 4);
        l.seed = o;    o += al((size_t)Nq * 4);
    }
    l.total = o;
    return l;
}

// err(d) = er * d + ea * (|q|^2 + max |r|^2) bounds |fp32 screened - fp64| distance.
//  * D <= 32, expanded form |q|^2 + q'.r' (or direct form at D = 16 / 32): <= 16 FMA roundings of
//    partial sums bounded by 2 (|q|^2 + |r|^2), plus the fp32 rounding of the inputs.  The MFMA
//    form without assuming fma-chain equivalence: each of the DP / 4 blocks adds 4 products to
//    the accumulator in any order, <= 1 rounding per product and per addition (5 per block), every
//    partial sum bounded by |q|^2 + sum |q'_j r'_j| <= 2 (|q|^2 + |r|^2); over 4 blocks
//    20 u * 2 (|q|^2 + |r|^2) = 40u (...), plus 4u (...) for the inputs: 44u = 2.7e-6 < ea = 4e-6
//    at DP = 16; at DP = 32 (8 blocks) 84u = 5.0e-6 < ea = 8e-6 (u = 2^-24);
//  * D > 32, direct form: D sequential FMAs of non-negative terms, each (q - r) rounded once:
//    relative (D + 3) u on the sum, plus 4 u (|q|^2 + |r|^2) from the inputs (u = 2^-24); 2x margin.
//
// Overflow guard.  These bounds are about finite fp32 numbers.  A screened distance that overflowed
// is +inf, or NaN in the expanded form (inf - inf, inf * 0 on a padding column); every screen drops
// such a row (`d < threshold` is false) without filling its list, so the merge would read "list not
// full: every row is in it" and certify an answer that lacks the row.  So the merge certifies a
// query only while S = |q|^2 + max |r|^2 < KNN_F32_SAFE = 2^125 (knn_internal.h; |q|^2 in fp64,
// max |r|^2 the fp32 norm from knn_convert, which is +inf as soon as a component or the norm
// overflowed), and sends it to the exhaustive fp64 scan otherwise.  Below that threshold nothing
// overflows, in either form and for every row r of the set:
//  * a converted component is at most sqrt(S), the expanded form's -2 r_c at most 2 sqrt(S), its
//    |r|^2 column at most S;
//  * direct form: (q_c - r_c)^2 <= 2 (q_c^2 + r_c^2), so every term and every partial sum is <= 2 S;
//  * expanded form: |q_c (-2 r_c)| <= q_c^2 + r_c^2, so |q|^2 plus any subset of the products, in
//    any order (inside an MFMA block too), plus |r|^2 is within +-(|q|^2 + S + |r|^2) <= 2 S;
//  * the roundings of the fp32 inputs, of the norms (a chain of <= 4096 FMAs) and of the partial
//    sums move each of these by a factor below 1 + 1e-3.
// 2 S (1 + 1e-3) < 2^126.01 against FLT_MAX ~ 2^128: a factor of almost 4 to spare.  The pilot
// and its seeds use the same arithmetic, so the same holds for them.  The guard is one fp64 add and
// compare per query on values the merge already holds.  It is about range only: NaN or infinite
// INPUTS are outside the contract (include/dsp_audiorec.h).
void knn_err_coeffs(const KnnLayout &l, int D, double &er, double &ea)
{
    if (!l.hd) {
        er = 2e-6;
        ea = l.DP <= 16 ? 4e-6 : 8e-6;
    } else {
        const double u = 1.0 / 16777216.0;
        er = 2.0 * (D + 3) * u * 1.05;
        ea = 2.0 * 4.2 * u;
    }
}
}  // namespace

extern "C" size_t dsp_knn_workspace_bytes(int64_t Nr, int64_t Nq, int D, int k)
{
    if (Nr < 0 || Nq < 0 || D < 1 || D > KNN_DMAX || k < 1 || k > 32) return 0;
    return knn_layout(Nr, Nq, D, k).total;
}

extern "C" size_t dsp_knn_workspace_fallbacks_offset(int64_t Nr, int64_t Nq, int D, int k)
{
    if (Nr < 0 || Nq < 0 || D < 1 || D > KNN_DMAX || k < 1 || k > 32) return 0;
    return knn_layout(Nr, Nq, D, k).misc + 4;
}

extern "C" int dsp_knn_classify(const double *ref, const int32_t *ref_labels, int64_t Nr,
                                const double *query, int64_t Nq, int D, int k, int64_t self_offset,
                                int n_classes, int32_t *idx, double *dist, int32_t *pred,
                                void *workspace, size_t workspace_bytes, int flags, void *stream)
{
    if (D < 1 || D > KNN_DMAX || k < 1 || k > dsp::KMAX || Nr < 0 || Nq < 0) return DSP_ERR_ARGS;
    if (Nr > 0x7fffffff || (Nq > 0 && (!query || !idx || !dist)) || (Nr > 0 && !ref))
        return DSP_ERR_ARGS;
    if (Nq == 0) return DSP_OK;
    (void)n_classes;
    const KnnLayout l = knn_layout(Nr, Nq, D, k);
    if (!workspace || workspace_bytes < l.total) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    float *ref32 = (float *)(ws + l.ref32);
    float *q32 = (float *)(ws + l.q32);
    float *cd = (float *)(ws + l.cand_d);
    int *ci = (int *)(ws + l.cand_i);
    unsigned *mx = (unsigned *)(ws + l.refmx);
    int *fbc = (int *)(ws + l.misc + 4);
    int *fbdone = (int *)(ws + l.misc + 16);
    int *fbl = (int *)(ws + l.misc + 16 + 4 * dsp::FB_C);
    float *seedp = l.rstride ? (float *)(ws + l.seed) : nullptr;
    if (hipMemsetAsync(ws + l.misc, 0, 16 + 4 * dsp::FB_C, s) != hipSuccess) return DSP_ERR_HIP;
    if (!(flags & DSP_KNN_REF_READY)) {  // (fit: the reference set in fp32 + its max norm)
        // an empty set too: the merge reads the max norm for its bound and its overflow guard
        if (hipMemsetAsync(mx, 0, 4, s) != hipSuccess) return DSP_ERR_HIP;
        if (Nr > 0) dsp::launch_knn_convert(s, ref, Nr, D, l.DP, l.exp ? 1 : 0, ref32, mx);
    }
    dsp::launch_knn_convert(s, query, Nq, D, l.DP, l.exp ? 2 : 0, q32, nullptr);
    if (l.hd) {
        dsp::launch_knn_screen_hd(s, l.DP, l.KC, l.nsplit, ref32, Nr, q32, Nq, self_offset, cd, ci);
    } else if (l.mfma) {
        if (l.rstride) {
            float seed_scale = 1.f;
#ifdef DSP_KNN_DIAG  // diagnostic build only: an adversarially tight seed (fallback tests)
            if (const char *e = getenv("DSP_KNN_SEED_SCALE")) seed_scale = (float)atof(e);
#endif
            // the pilot over the sampled rows (same fp32 arithmetic as the screen), whose seeds
            // start the screen
            float *pd = (float *)(ws + l.pilot_d);
            dsp::launch_knn_pilot(s, l.DP, l.nsplit_p, ref32, l.nsample, l.rstride, q32, Nq, self_offset, pd);
            dsp::launch_knn_seed(s, l.KC, pd, l.nsplit_p, Nq, seedp, seed_scale);
        }
        dsp::launch_knn_screen_mfma(s, l.DP, l.KC, l.nsplit, ref32, Nr, q32, Nq, self_offset, cd, ci, seedp);
    } else {
        dsp::launch_knn_screen(s, l.DP, l.KC, l.nsplit, ref32, Nr, q32, Nq, self_offset, cd, ci);
    }
    double er, ea;
    knn_err_coeffs(l, D, er, ea);
    const int32_t *lbl = pred ? ref_labels : nullptr;
    if (!dsp::launch_knn_merge(s, l.KC, ref, query, Nr, Nq, D, k, l.nsplit, self_offset, cd, ci, mx, er, ea, lbl, idx,
                               dist, pred, fbc, fbl, seedp))
        return DSP_ERR_ARGS;  // unreachable while KC >= k + KNN_SLACK (knn_layout)
    dsp::launch_knn_fallback(s, l.fb_km, ref, query, Nr, Nq, D, k, self_offset, fbc, fbl, lbl, idx, dist, pred,
                             l.fb_parts, (double *)(ws + l.fb_d), (int *)(ws + l.fb_i), fbdone);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
}

extern "C" int dsp_abi_version(void) { return DSP_ABI_VERSION; }
