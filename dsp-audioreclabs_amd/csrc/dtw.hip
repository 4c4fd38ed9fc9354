// dtw.hip -- dynamic time warping between padded frame sequences and the k nearest neighbours
// under it, on gfx950 (include/dsp_audiorec.h: dsp_dtw_pairwise, dsp_dtw_knn).
//
// Definition.  a is [Nq, Tq, F] with len_a [Nq], b is [Nr, Tr, F] with len_b [Nr], float64, padded
// row-major.  For a pair with lengths n, m:
//   c(i,j) = sum_f (a[i,f] - b[j,f])^2        f ascending, fp64, each product and each sum rounded
//   D(0,0) = c(0,0)
//   D(i,j) = c(i,j) + min(D(i-1,j), D(i,j-1), D(i-1,j-1))   neighbours outside the grid or the band: +inf
//   dtw    = sqrt(D(n-1, m-1))
// window < 0: unconstrained; window >= 0: cell (i,j) is admissible iff |i - j| <= max(window, |n - m|)
// (a Sakoe-Chiba band that always reaches the end cell).  Only fp64 subtract, multiply, add, min and
// sqrt occur, all correctly rounded, and min is order-independent on non-negative finite values: the
// result is defined bit for bit.  (a - b)^2 == (b - a)^2 exactly, so dtw(a, b) and dtw(b, a) have
// equal bits and the kernel is free to walk the grid transposed.  A sequence whose length is < 1
// or greater than its padded width has distance +inf to everything.
//
// Three kernels:
//   dtw_dp<F>  one wave per tile of 64 reference sequences against ONE query (a workgroup is one
//              wave): dtw_internal.h's sweep with the query as the uniform side and a lane per
//              reference.  Waves are persistent: a launch has at most DTW_WAVES of them, each
//              walking tiles wave, wave + G, ... so the edge arrays are bounded.
//   dtw_pad    the padded copy of a chunk of uniform-side sequences that the sweep reads (also
//              dtw_align.hip's, through dtw_launch_pad).
//   dtw_topk   one wave per query over that query's distance row: k rounds of "the smallest
//              (distance, index) pair after the last one taken", a butterfly minimum per round.
//              Negligible next to the DP.  The vote is dsp_knn_classify's: uniform, the smallest
//              label among the most frequent.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dsp_audiorec.h"
#include "dtw_internal.h"  // the plan, the row body and the sweep (shared with dtw_align.hip)

namespace dsp {

static constexpr int DTW_KMAX = 32;                   // largest k
static constexpr size_t DTW_EDGE_CAP = 256u << 20;    // bytes of edge arrays per launch
static constexpr size_t DTW_CHUNK_CAP = 64u << 20;    // bytes of distance rows per query chunk
static constexpr int DTW_QCHUNK = 1024;               // queries per chunk at most

// apad [Nq, Tq + DTW_STRIP, F]: DTW_STRIP frames of zeros, then a's row -- the first strip of an
// end-aligned walk starts up to 31 frames before frame 0, and reads them here instead of outside the row
__global__ __launch_bounds__(256) void dtw_pad(const double *__restrict__ a, int64_t Nq, int Tq, int F,
                                               double *__restrict__ apad)
{
    const int64_t rowp = (int64_t)(Tq + DTW_STRIP) * F, total = Nq * rowp;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t q = i / rowp, e = i - q * rowp - (int64_t)DTW_STRIP * F;
        apad[i] = e < 0 ? 0.0 : a[q * Tq * F + e];
    }
}
void dtw_launch_pad(hipStream_t s, const double *in, int64_t rows, int T, int F, double *out)
{
    const int64_t elems = rows * (T + DTW_STRIP) * F;
    hipLaunchKernelGGL(dtw_pad, dim3((unsigned)std::min<int64_t>((elems + 255) / 256, 4096)), dim3(256), 0, s, in, rows,
                       T, F, out);
}

// apad: the uniform side (one sequence per tile, padded by dtw_pad), b: the lanes' side.  dist [Nq, Nr].
template <int F>
__global__ __launch_bounds__(64) void dtw_dp(const double *__restrict__ apad, const int32_t *__restrict__ len_a,
                                             int64_t Nq, int Tq, const double *__restrict__ b,
                                             const int32_t *__restrict__ len_b, int64_t Nr, int Tr, int window,
                                             double *__restrict__ dist, double *__restrict__ edge_ws)
{
    const int lane = (int)threadIdx.x;
    const int64_t nrb = (Nr + 63) / 64, ntiles = Nq * nrb;
    // this wave's edge column, [row][lane]; only sequences longer than one strip use it
    double *__restrict__ edge = edge_ws + (size_t)blockIdx.x * (size_t)Tr * 64 + lane;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t uq = tile / nrb, ref = (tile - uq * nrb) * 64 + lane;
        const bool inr = ref < Nr;
        const int n = len_a[uq];
        int m = inr ? len_b[ref] : 0;
        if (m < 1 || m > Tr) m = 0;
        double res = INFINITY;
        const int mmax = wave_max_uniform(m);
        if (n >= 1 && n <= Tq && mmax > 0)
            res = dtw_sweep<F, false>(apad + (uq * (Tq + DTW_STRIP) + DTW_STRIP) * F,  // frame 0
                                      b + (inr ? ref : 0) * (int64_t)Tr * F, n, m, mmax, window, Tr, edge, nullptr);
        if (inr) dist[uq * Nr + ref] = res < INFINITY ? sqrt(res) : (double)INFINITY;
    }
}

__device__ __forceinline__ bool dtw_less(double da, int ia, double db, int ib)
{
    return da < db || (da == db && ia < ib);
}

// rows: nq distance rows [nq, Nr] of the queries q0 .. q0 + nq; outputs indexed by the query number
__global__ __launch_bounds__(64) void dtw_topk(const double *__restrict__ rows, int64_t nq, int64_t Nr, int k,
                                               int64_t q0, int64_t self_offset, const int32_t *__restrict__ labels,
                                               int32_t *__restrict__ idx, double *__restrict__ dist,
                                               int32_t *__restrict__ pred)
{
    const int lane = (int)threadIdx.x;
    for (int64_t qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        const double *__restrict__ d = rows + qi * Nr;
        const int64_t q = q0 + qi;
        const int64_t self = self_offset >= 0 ? self_offset + q : -1;
        double ld = -1.0, myd = INFINITY;  // (ld, li): the pair taken last; distances are >= 0
        int li = -1, myi = -1;
        for (int j = 0; j < k; j++) {
            double bd = INFINITY;
            int bi = 0x7fffffff;
            for (int64_t r = lane; r < Nr; r += 64) {
                const double v = d[r];
                if (r == self || !(v < INFINITY)) continue;
                if (dtw_less(ld, li, v, (int)r) && dtw_less(v, (int)r, bd, bi)) {
                    bd = v;
                    bi = (int)r;
                }
            }
#pragma unroll
            for (int msk = 1; msk < 64; msk <<= 1) {
                const double od = __shfl_xor(bd, msk, 64);
                const int oi = __shfl_xor(bi, msk, 64);
                if (dtw_less(od, oi, bd, bi)) {
                    bd = od;
                    bi = oi;
                }
            }
            if (lane == j) {
                myd = bd;
                myi = bd < INFINITY ? bi : -1;
            }
            ld = bd;  // exhausted: (inf, max) -- nothing comes after it
            li = bi;
        }
        if (lane < k) {
            idx[q * k + lane] = myi;
            dist[q * k + lane] = myd;
        }
        if (pred && labels) {  // dsp_knn_classify's vote: uniform, the smallest most frequent label
            const int lab = (lane < k && myi >= 0) ? labels[myi] : -1;
            int best = -1, bestc = 0;
            for (int x = 0; x < k; x++) {
                const int la = __shfl(lab, x, 64);
                if (la < 0) continue;
                int cnt = 0;
                for (int y = 0; y < k; y++) cnt += __shfl(lab, y, 64) == la;
                if (cnt > bestc || (cnt == bestc && la < best)) {
                    bestc = cnt;
                    best = la;
                }
            }
            if (lane == 0) pred[q] = best;
        }
    }
}

// ---- host side ----
static bool dtw_in_plan(int64_t Nr, int64_t Nq, int Tr, int Tq, int F)
{
    return Nr >= 0 && Nr <= 0x7fffffff && Nq >= 0 && dtw_shape_in_plan(Tr, Tq, F);
}
// waves of a launch over nq queries, and the bytes of their edge arrays
static int dtw_waves(int64_t nq, int64_t Nr, int Tr)
{
    const int64_t ntiles = nq * ((Nr + 63) / 64);
    const int64_t cap = std::max<int64_t>(1, (int64_t)(DTW_EDGE_CAP / ((size_t)Tr * 64 * 8)));
    return (int)std::min<int64_t>(ntiles, std::min<int64_t>(DTW_WAVES, cap));
}
static size_t dtw_edge_bytes(int64_t nq, int64_t Nr, int Tr, int Tq)
{
    if (Tq <= DTW_STRIP) return 256;  // one strip: no edge is ever read or written
    return up256((size_t)dtw_waves(nq, Nr, Tr) * Tr * 64 * 8);
}
static int64_t dtw_chunk(int64_t Nr, int64_t Nq)
{
    const int64_t by_bytes = std::max<int64_t>(1, (int64_t)(DTW_CHUNK_CAP / (8 * (size_t)std::max<int64_t>(Nr, 1))));
    return std::max<int64_t>(1, std::min<int64_t>(Nq, std::min<int64_t>(DTW_QCHUNK, by_bytes)));
}

// one chunk: pad its queries, then the DP
static int dtw_launch_dp(hipStream_t s, const double *a_rows, const int32_t *len_a, int64_t nq, int Tq,
                         const double *b, const int32_t *len_b, int64_t Nr, int Tr, int F, int window, double *dist,
                         double *edge, double *a)
{
    const int G = dtw_waves(nq, Nr, Tr);
    if (G < 1) return DSP_OK;
    dtw_launch_pad(s, a_rows, nq, Tq, F, a);
    DTW_LAUNCH_F(F, dtw_dp, dim3((unsigned)G), dim3(64), 0, s, a, len_a, nq, Tq, b, len_b, Nr, Tr, window, dist, edge)
    return dtw_launch_status();
}

}  // namespace dsp

// workspace: [edge columns of one chunk's waves][the chunk's padded queries][the chunk's distance rows]
extern "C" size_t dsp_dtw_workspace_bytes(int64_t Nr, int64_t Nq, int Tr, int Tq, int F, int k)
{
    if (!dsp::dtw_in_plan(Nr, Nq, Tr, Tq, F) || k < 1 || k > dsp::DTW_KMAX) return 0;
    const int64_t chunk = dsp::dtw_chunk(Nr, Nq);
    return dsp::dtw_edge_bytes(chunk, Nr, Tr, Tq) + dsp::dtw_pad_bytes(chunk, Tq, F) +
           (size_t)chunk * (size_t)std::max<int64_t>(Nr, 1) * 8;
}

// the queries in chunks: DP into rows (k > 0, then the top-k) or straight into dist [Nq, Nr] (k == 0)
static int dtw_run(const double *ref, const int32_t *len_ref, const int32_t *ref_labels, int64_t Nr, int Tr,
                   const double *query, const int32_t *len_query, int64_t Nq, int Tq, int F, int window, int k,
                   int64_t self_offset, int32_t *idx, double *dist, int32_t *pred, void *workspace, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int64_t chunk = dsp::dtw_chunk(Nr, Nq);
    double *edge = (double *)workspace;
    double *pad = (double *)((char *)workspace + dsp::dtw_edge_bytes(chunk, Nr, Tr, Tq));
    double *rows = (double *)((char *)pad + dsp::dtw_pad_bytes(chunk, Tq, F));
    for (int64_t q0 = 0; q0 < Nq; q0 += chunk) {
        const int64_t nq = std::min(chunk, Nq - q0);
        if (Nr > 0) {
            const int rc = dsp::dtw_launch_dp(s, query + q0 * Tq * F, len_query + q0, nq, Tq, ref, len_ref, Nr, Tr, F,
                                              window, k > 0 ? rows : dist + q0 * Nr, edge, pad);
            if (rc != DSP_OK) return rc;
        }
        if (k < 1) continue;
        hipLaunchKernelGGL(dsp::dtw_topk, dim3((unsigned)std::min<int64_t>(nq, 65536)), dim3(64), 0, s, rows, nq, Nr,
                           k, q0, self_offset, ref_labels, idx, dist, pred);
        const int rc = dsp::dtw_launch_status();
        if (rc != DSP_OK) return rc;
    }
    return DSP_OK;
}

extern "C" int dsp_dtw_pairwise(const double *a, const int32_t *len_a, int64_t Nq, int Tq, const double *b,
                                const int32_t *len_b, int64_t Nr, int Tr, int F, int window, double *dist,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    if (!dsp::dtw_in_plan(Nr, Nq, Tr, Tq, F)) return DSP_ERR_ARGS;
    if (Nq == 0 || Nr == 0) return DSP_OK;
    if (!a || !len_a || !b || !len_b || !dist) return DSP_ERR_ARGS;
    const int64_t chunk = dsp::dtw_chunk(Nr, Nq);
    if (!workspace || workspace_bytes < dsp::dtw_edge_bytes(chunk, Nr, Tr, Tq) + dsp::dtw_pad_bytes(chunk, Tq, F))
        return DSP_ERR_WORKSPACE;
    return dtw_run(b, len_b, nullptr, Nr, Tr, a, len_a, Nq, Tq, F, window, 0, -1, nullptr, dist, nullptr, workspace,
                   stream);
}

extern "C" int dsp_dtw_knn(const double *ref, const int32_t *len_ref, const int32_t *ref_labels, int64_t Nr, int Tr,
                           const double *query, const int32_t *len_query, int64_t Nq, int Tq, int F, int window,
                           int k, int64_t self_offset, int n_classes, int32_t *idx, double *dist, int32_t *pred,
                           void *workspace, size_t workspace_bytes, void *stream)
{
    (void)n_classes;
    if (!dsp::dtw_in_plan(Nr, Nq, Tr, Tq, F) || k < 1 || k > dsp::DTW_KMAX) return DSP_ERR_ARGS;
    if (Nq == 0) return DSP_OK;
    if (!query || !len_query || !idx || !dist || (Nr > 0 && (!ref || !len_ref))) return DSP_ERR_ARGS;
    if (!workspace || workspace_bytes < dsp_dtw_workspace_bytes(Nr, Nq, Tr, Tq, F, k)) return DSP_ERR_WORKSPACE;
    return dtw_run(ref, len_ref, ref_labels, Nr, Tr, query, len_query, Nq, Tq, F, window, k, self_offset, idx, dist,
                   pred, workspace, stream);
}
