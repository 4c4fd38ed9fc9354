// svm.hip -- SVC(kernel='rbf').predict on gfx950 (include/dsp_audiorec.h: dsp_svc_predict), the
// prediction side of the reference's TraditionalClassifier('svm') (src/models.py:44-47, :56-58).
// Training stays libsvm's; a fitted model is a fixed set of support vectors, dual
// coefficients and intercepts, and libsvm's predict is
//   K_s   = exp(-gamma * sum_d (q_d - sv_{s,d})^2)
//   dec_p = sum_{s in class i} coef[j-1][s] K_s + sum_{s in class j} coef[i][s] K_s + intercept[p]
//           for the pairs i < j in libsvm's order p
//   vote  i if dec_p > 0 else j; the first class with the most votes wins.
// Put differently, a support vector of class c adds coef[r][s] K_s to the pair of c with class
// o = r if r < c else r + 1: walking the support vectors class by class needs C - 1 accumulators
// per query ("class block" (c, r)), and dec of the pair i < j is block(i, j-1) + block(j, i) + b.
//
// Three kernels, all fp64, fixed summation order, no atomics on floating-point data:
//   svc_prep    cmax[s] = max_r |coef[r][s]| and A = sum_s cmax[s] (the certification's weights)
//   svc_main    a lane owns one query; tiles of support vectors with their coefficient columns and
//               cmax in LDS, read as broadcasts; class blocks and B_q = sum_s cmax[s] K_s out
//   svc_finish  sums the parts in index order, forms dec_p, certifies, votes, counts uncertified
//
// Canonical summation order.  Every class's support vectors are cut into G segments, G a function
// of nSV alone: segment g of a class of n rows is rows [n g / G, n (g+1) / G).  A segment is summed
// from zero in row order; a class block is the sum of its segments' sums in segment order.  A
// workgroup of the query-tiled launch walks all G segments and keeps that running sum; the
// SV-split launch (few queries against many support vectors) gives each segment its own workgroup,
// writes G parts, and svc_finish adds them in the same order.  So a query's dec bits do not depend
// on which launch ran, on Nq, or on the query's position in the batch.
//
// Certification: |dec_device - dec_libsvm| <= bound_p for any summation order on
// both sides,
//   bound_p = 2^-52 [ (n_i + n_j + 4) (B_q + |b_p|) + 2 SVC_EXP_ULPS B_q + (D + 4) A / e ]
// and a query is certified when every pair has |dec_p| > SVC_SAFETY bound_p.  The caller answers
// the others with libsvm itself.  A row holding an inf or a NaN is never certified (svc_main).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsp_audiorec.h"

namespace dsp {

static constexpr int SVC_T = 128;      // queries per workgroup (one per lane)
static constexpr int SVC_TS = 32;      // support vectors per LDS tile
static constexpr int SVC_HD_S = 16;    // D > 32: support vectors per tile ...
static constexpr int SVC_HD_C = 16;    // ... and dimensions per chunk
static constexpr int SVC_SEG_ROWS = 256;  // G = ceil(nSV / SVC_SEG_ROWS), at most SVC_GMAX
static constexpr int SVC_GMAX = 64;
static constexpr double SVC_EXP_ULPS = 4.0;  // allowance per exp, each side (ocml's and glibc's are < 1)
static constexpr double SVC_SAFETY = 4.0;
static constexpr double SVC_INV_E = 0.36787944117144233;  // max x e^-x, rounded up

// cmax[s] = max_r |coef[r][s]|; asum[0] = sum_s cmax[s] (one workgroup, fixed order).  It also zeroes
// the uncertified count for svc_finish: a kernel's store, not hipMemsetAsync, so that a captured call
// is a plain chain of kernels (after a graph replay the memset's counter did not read as zeroed).
__global__ __launch_bounds__(256) void svc_prep(const double *__restrict__ coef, int64_t nSV, int C,
                                                double *__restrict__ cmax, double *__restrict__ asum,
                                                int32_t *__restrict__ uncertified)
{
    __shared__ double red[256];
    double a = 0.0;
    for (int64_t s = threadIdx.x; s < nSV; s += 256) {
        double m = 0.0;
        for (int r = 0; r < C - 1; r++) m = fmax(m, fabs(coef[(int64_t)r * nSV + s]));
        cmax[s] = m;
        a += m;
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        asum[0] = red[0];
        uncertified[0] = 0;
    }
}

struct SvcArgs {
    const double *sv, *coef, *cmax, *query;
    const int32_t *nsup;
    int64_t nSV, Nq;
    int D, C, G;
    double gamma;
    double *part;  // [parts][C (C-1)][Nq]
    double *bq;    // [parts][C][Nq]
};

// rows [lo, hi) of segment g of a class of n rows starting at row `start`, clamped into the model
__device__ __forceinline__ void svc_segment(int64_t start, int n, int g, int G, int64_t nSV, int64_t &lo, int64_t &hi)
{
    lo = start + (int64_t)n * g / G;
    hi = start + (int64_t)n * (g + 1) / G;
    hi = hi < nSV ? hi : nSV;
    lo = lo > 0 ? lo : 0;
    lo = lo < hi ? lo : hi;
}

// one support vector's share: K into the class block's CR rows and into B_q
template <int CR>
__device__ __forceinline__ void svc_accumulate(double K, const double *cf, double cm, double (&seg)[CR],
                                               double &bseg)
{
    bseg = fma(cm, K, bseg);
#pragma unroll
    for (int r = 0; r < CR; r++) seg[r] = fma(cf[r], K, seg[r]);
}

// DP = 16 / 32: D <= DP, the query in registers (columns D.. are zero on both sides).  DP = 0:
// D > 32, the dimensions walked in chunks of SVC_HD_C with SVC_HD_S running distances per lane.
// CR >= C - 1 coefficient rows (rows C-1.. are zero).
template <int DP, int CR>
__global__ __launch_bounds__(SVC_T) void svc_main(const SvcArgs a)
{
    constexpr bool HD = DP == 0;
    constexpr int TS = HD ? SVC_HD_S : SVC_TS;
    constexpr int COLS = HD ? SVC_HD_C : DP;
    __shared__ double s_sv[TS * COLS];
    __shared__ double s_cf[TS * CR];
    __shared__ double s_cm[TS];

    const int tid = threadIdx.x;
    const int64_t q_raw = (int64_t)blockIdx.x * SVC_T + tid;
    const bool live = q_raw < a.Nq;
    const int64_t qi = live ? q_raw : a.Nq - 1;  // idle lanes shadow the last query (barriers are block-wide)
    const int part = blockIdx.y;
    const int g0 = gridDim.y > 1 ? part : 0, g1 = gridDim.y > 1 ? part + 1 : a.G;
    const int C = a.C, D = a.D;
    const double *qrow = a.query + qi * D;

    double q[HD ? 1 : DP];
    if constexpr (!HD) {
#pragma unroll
        for (int d = 0; d < DP; d++) q[d] = d < D ? qrow[d] : 0.0;
    }
    // A row holding an inf would give d^2 = inf, K_s = 0 and dec_p = intercept[p] with a small bound:
    // certified, where libsvm's caller refuses the row.  x * 0 is NaN for an inf and for a NaN and +0
    // (after the add) for every finite x, so the lane's class blocks and B_q start from `poison`
    // instead of zero: a finite row keeps its bits, any other gets NaN in every dec_p and in its bound.
    double poison = 0.0;
    if constexpr (!HD) {
#pragma unroll
        for (int d = 0; d < DP; d++) poison = fma(q[d], 0.0, poison);
    } else {
        for (int d = 0; d < D; d++) poison = fma(qrow[d], 0.0, poison);
    }

    int64_t start = 0;
    for (int c = 0; c < C; c++) {
        const int n = a.nsup[c];
        double total[CR], btotal = poison;
#pragma unroll
        for (int r = 0; r < CR; r++) total[r] = poison;
        for (int g = g0; g < g1; g++) {
            int64_t lo, hi;
            svc_segment(start, n, g, a.G, a.nSV, lo, hi);
            double seg[CR], bseg = 0.0;
#pragma unroll
            for (int r = 0; r < CR; r++) seg[r] = 0.0;
            for (int64_t t0 = lo; t0 < hi; t0 += TS) {
                const int nt = (int)(hi - t0 < TS ? hi - t0 : TS);
                if constexpr (!HD) {
                    __syncthreads();  // the previous tile is consumed
                    for (int e = tid; e < TS * DP; e += SVC_T) {
                        const int s = e / DP, d = e % DP;
                        s_sv[e] = (s < nt && d < D) ? a.sv[(t0 + s) * D + d] : 0.0;
                    }
                    for (int e = tid; e < TS * CR; e += SVC_T) {
                        const int s = e / CR, r = e % CR;
                        s_cf[e] = (s < nt && r < C - 1) ? a.coef[(int64_t)r * a.nSV + t0 + s] : 0.0;
                    }
                    if (tid < TS) s_cm[tid] = tid < nt ? a.cmax[t0 + tid] : 0.0;
                    __syncthreads();
                    for (int s = 0; s < nt; s++) {
                        double d2 = 0.0;
#pragma unroll
                        for (int d = 0; d < DP; d++) {
                            const double diff = q[d] - s_sv[s * DP + d];
                            d2 = fma(diff, diff, d2);
                        }
                        svc_accumulate<CR>(exp(-(a.gamma * d2)), &s_cf[s * CR], s_cm[s], seg, bseg);
                    }
                } else {
                    double d2[TS];
#pragma unroll
                    for (int s = 0; s < TS; s++) d2[s] = 0.0;
                    for (int d0 = 0; d0 < D; d0 += COLS) {
                        double qc[COLS];
#pragma unroll
                        for (int j = 0; j < COLS; j++) qc[j] = d0 + j < D ? qrow[d0 + j] : 0.0;
                        __syncthreads();  // the previous chunk (and tile) is consumed
                        for (int e = tid; e < TS * COLS; e += SVC_T) {
                            const int s = e / COLS, d = d0 + e % COLS;
                            s_sv[e] = (s < nt && d < D) ? a.sv[(t0 + s) * D + d] : 0.0;
                        }
                        if (d0 == 0) {
                            for (int e = tid; e < TS * CR; e += SVC_T) {
                                const int s = e / CR, r = e % CR;
                                s_cf[e] = (s < nt && r < C - 1) ? a.coef[(int64_t)r * a.nSV + t0 + s] : 0.0;
                            }
                            if (tid < TS) s_cm[tid] = tid < nt ? a.cmax[t0 + tid] : 0.0;
                        }
                        __syncthreads();
#pragma unroll
                        for (int s = 0; s < TS; s++) {
#pragma unroll
                            for (int j = 0; j < COLS; j++) {
                                const double diff = qc[j] - s_sv[s * COLS + j];
                                d2[s] = fma(diff, diff, d2[s]);
                            }
                        }
                    }
#pragma unroll
                    for (int s = 0; s < TS; s++)
                        if (s < nt) svc_accumulate<CR>(exp(-(a.gamma * d2[s])), &s_cf[s * CR], s_cm[s], seg, bseg);
                }
            }
#pragma unroll
            for (int r = 0; r < CR; r++) total[r] += seg[r];
            btotal += bseg;
        }
        if (live) {
            const int64_t base = ((int64_t)part * C * (C - 1) + (int64_t)c * (C - 1)) * a.Nq + q_raw;
#pragma unroll
            for (int r = 0; r < CR; r++)
                if (r < C - 1) a.part[base + (int64_t)r * a.Nq] = total[r];
            a.bq[((int64_t)part * C + c) * a.Nq + q_raw] = btotal;
        }
        start += n;
    }
}

struct SvcFinishArgs {
    const double *part, *bq, *intercept, *asum;
    const int32_t *nsup;
    int64_t Nq;
    int D, C, parts;
    int32_t *pred, *certified, *uncertified;
    double *dec;  // [Nq][C (C-1) / 2] or NULL
};

// class block (c, r) of query q: its parts in index order
__device__ __forceinline__ double svc_block(const SvcFinishArgs &a, int c, int r, int64_t q)
{
    double v = 0.0;
    for (int p = 0; p < a.parts; p++) v += a.part[(((int64_t)p * a.C + c) * (a.C - 1) + r) * a.Nq + q];
    return v;
}
// dec of the pair i < j (libsvm index p): the one expression both visits of the pair evaluate
__device__ __forceinline__ double svc_dec(const SvcFinishArgs &a, int i, int j, int p, int64_t q)
{
    return (svc_block(a, i, j - 1, q) + svc_block(a, j, i, q)) + a.intercept[p];
}

__global__ __launch_bounds__(256) void svc_finish(const SvcFinishArgs a)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.Nq) return;
    const int C = a.C;
    double B = 0.0;
    for (int c = 0; c < C; c++) {
        double b = 0.0;
        for (int p = 0; p < a.parts; p++) b += a.bq[((int64_t)p * C + c) * a.Nq + q];
        B += b;
    }
    const double dist_term = (double)(a.D + 4) * a.asum[0] * SVC_INV_E;
    // class i's votes: pairs (i, j > i) with dec > 0 and pairs (j < i, i) with dec <= 0 -- every pair
    // is formed twice, by the same expression, so no per-class counters are kept
    bool cert = true;
    int best = 0, best_votes = -1;
    for (int i = 0; i < C; i++) {
        int votes = 0;
        for (int j = 0; j < C; j++) {
            if (j == i) continue;
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            const int p = lo * (2 * C - lo - 1) / 2 + (hi - lo - 1);
            const double d = svc_dec(a, lo, hi, p, q);
            votes += (d > 0.0) == (i < j) ? 1 : 0;
            if (i < j) {
                if (a.dec) a.dec[q * ((int64_t)C * (C - 1) / 2) + p] = d;
                const double bp = fabs(a.intercept[p]);
                const double bound = 0x1p-52 * ((double)(a.nsup[i] + a.nsup[j] + 4) * (B + bp) +
                                                2.0 * SVC_EXP_ULPS * B + dist_term);
                cert = cert && (fabs(d) > SVC_SAFETY * bound);  // (false for a NaN)
            }
        }
        if (votes > best_votes) {
            best_votes = votes;
            best = i;
        }
    }
    a.pred[q] = best;
    a.certified[q] = cert ? 1 : 0;
    if (!cert) atomicAdd(a.uncertified, 1);
}

}  // namespace dsp

namespace {
static constexpr int SVC_DMAX = 4096, SVC_CMAX = 64;
static constexpr int64_t SVC_SPLIT_MAX_NQ = 512;         // the SV-split launch: at most this many queries ...
static constexpr size_t SVC_SPLIT_MAX_BYTES = 64u << 20;  // ... and this much for its parts

struct SvcLayout {
    size_t cmax, asum, count, part, bq, total;
    int G, parts;
};

size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

bool svc_args_ok(int64_t nSV, int64_t Nq, int D, int C)
{
    return nSV >= 1 && nSV <= 0x7fffffff && Nq >= 0 && D >= 1 && D <= SVC_DMAX && C >= 2 && C <= SVC_CMAX;
}

// sizes only: two launches of the same shape take the same path
SvcLayout svc_layout(int64_t nSV, int64_t Nq, int D, int C)
{
    SvcLayout l;
    (void)D;
    int64_t G = (nSV + dsp::SVC_SEG_ROWS - 1) / dsp::SVC_SEG_ROWS;
    l.G = (int)(G < 1 ? 1 : G > dsp::SVC_GMAX ? dsp::SVC_GMAX : G);
    const size_t per_part = (size_t)C * (C - 1) * (size_t)Nq * 8;
    l.parts = (l.G > 1 && Nq <= SVC_SPLIT_MAX_NQ && per_part * l.G <= SVC_SPLIT_MAX_BYTES) ? l.G : 1;
    l.cmax = 0;
    l.asum = al((size_t)nSV * 8);
    l.count = l.asum + 8;
    l.part = l.asum + 256;
    l.bq = l.part + al(per_part * l.parts);
    l.total = l.bq + al((size_t)l.parts * C * (size_t)Nq * 8);
    return l;
}

template <int DP>
void svc_launch(int C, dim3 grid, hipStream_t s, const dsp::SvcArgs &a)
{
    if (C <= 2) hipLaunchKernelGGL((dsp::svc_main<DP, 1>), grid, dim3(dsp::SVC_T), 0, s, a);
    else if (C <= 4) hipLaunchKernelGGL((dsp::svc_main<DP, 3>), grid, dim3(dsp::SVC_T), 0, s, a);
    else if (C <= 10) hipLaunchKernelGGL((dsp::svc_main<DP, 9>), grid, dim3(dsp::SVC_T), 0, s, a);
    else if (C <= 32) hipLaunchKernelGGL((dsp::svc_main<DP, 31>), grid, dim3(dsp::SVC_T), 0, s, a);
    else hipLaunchKernelGGL((dsp::svc_main<DP, 63>), grid, dim3(dsp::SVC_T), 0, s, a);
}
}  // namespace

extern "C" size_t dsp_svc_workspace_bytes(int64_t nSV, int64_t Nq, int D, int C)
{
    if (!svc_args_ok(nSV, Nq, D, C)) return 0;
    return svc_layout(nSV, Nq, D, C).total;
}

extern "C" size_t dsp_svc_workspace_uncertified_offset(int64_t nSV, int64_t Nq, int D, int C)
{
    if (!svc_args_ok(nSV, Nq, D, C)) return 0;
    return svc_layout(nSV, Nq, D, C).count;
}

extern "C" int dsp_svc_launch_parts(int64_t nSV, int64_t Nq, int D, int C)
{
    if (!svc_args_ok(nSV, Nq, D, C)) return 0;
    return svc_layout(nSV, Nq, D, C).parts;
}

extern "C" int dsp_svc_predict(const double *sv, const int32_t *n_support, const double *dual_coef,
                               const double *intercept, int64_t nSV, int D, int C, double gamma,
                               const double *query, int64_t Nq, int32_t *pred, double *dec,
                               int32_t *certified, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!svc_args_ok(nSV, Nq, D, C) || !(gamma >= 0.0) || !sv || !n_support || !dual_coef || !intercept)
        return DSP_ERR_ARGS;
    if (Nq > 0 && (!query || !pred || !certified)) return DSP_ERR_ARGS;
    if (Nq == 0) return DSP_OK;
    const SvcLayout l = svc_layout(nSV, Nq, D, C);
    if (!workspace || workspace_bytes < l.total) return DSP_ERR_WORKSPACE;
    const int64_t qtiles = (Nq + dsp::SVC_T - 1) / dsp::SVC_T, fblocks = (Nq + 255) / 256;
    if (qtiles > 0x7fffffff) return DSP_ERR_ARGS;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    double *cmax = (double *)(ws + l.cmax), *asum = (double *)(ws + l.asum);
    hipLaunchKernelGGL(dsp::svc_prep, dim3(1), dim3(256), 0, s, dual_coef, nSV, C, cmax, asum,
                       (int32_t *)(ws + l.count));

    dsp::SvcArgs a;
    a.sv = sv, a.coef = dual_coef, a.cmax = cmax, a.query = query, a.nsup = n_support;
    a.nSV = nSV, a.Nq = Nq, a.D = D, a.C = C, a.G = l.G, a.gamma = gamma;
    a.part = (double *)(ws + l.part), a.bq = (double *)(ws + l.bq);
    const dim3 grid((unsigned)qtiles, (unsigned)l.parts);
    if (D <= 16) svc_launch<16>(C, grid, s, a);
    else if (D <= 32) svc_launch<32>(C, grid, s, a);
    else svc_launch<0>(C, grid, s, a);

    dsp::SvcFinishArgs f;
    f.part = a.part, f.bq = a.bq, f.intercept = intercept, f.asum = asum, f.nsup = n_support;
    f.Nq = Nq, f.D = D, f.C = C, f.parts = l.parts;
    f.pred = pred, f.certified = certified, f.uncertified = (int32_t *)(ws + l.count), f.dec = dec;
    hipLaunchKernelGGL(dsp::svc_finish, dim3((unsigned)fblocks), dim3(256), 0, s, f);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
}
