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
//              wave).  Lane l owns the pair (query, reference l); the query's frames are the same
//              for every lane, so they are read with wave-uniform addresses (scalar loads, no LDS
//              and no vector-memory traffic per cell), and only the lane's own reference frame --
//              F values per DP row -- comes through the vector path, prefetched one row ahead.
//              The lane keeps a strip of 32 DP cells (32 consecutive query frames) in registers and
//              sweeps its reference's frames in the outer loop, the strip loop fully unrolled so
//              the register array is never indexed at run time.  Strips are END-aligned (the last
//              one ends at query frame n - 1, the first may start before frame 0 with those cells
//              held at +inf), so the strip's last register is both the edge handed to the next
//              strip and, in the last strip, the result; dtw_pad first copies the chunk's queries
//              behind 32 frames of zeros, so those reads stay inside the copy's row and every
//              strip reads its 32 query frames at constant offsets from one base.  A strip hands
//              its edge column D(., last) to the next one through a per-wave array in the
//              workspace laid out [row][lane] (coalesced); the first strip reads +inf, the last
//              writes nothing.
//              Loop bounds are wave-uniform (the largest reference length and band of the wave's
//              lanes); rows past a lane's own length compute values nothing reads.  Rows of a strip
//              that are admissible for no lane are skipped; a row that is admissible in all its 32
//              cells for every lane runs a body without the band select (row 0, with the start
//              cell, has a body of its own).  Waves are persistent: a launch has at most
//              DTW_WAVES of them, each walking tiles wave, wave + G, ... so the edge arrays are
//              bounded.
//   dtw_pad    the padded copy of a chunk of queries (above).
//   dtw_topk   one wave per query over that query's distance row: k rounds of "the smallest
//              (distance, index) pair after the last one taken", a butterfly minimum per round.
//              Negligible next to the DP.  The vote is dsp_knn_classify's: uniform, the smallest
//              label among the most frequent.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dsp_audiorec.h"
#include "dtw_internal.h"  // the plan's constants, wave_max_uniform, dtw_min (shared with dtw_align.hip)

namespace dsp {

static constexpr int DTW_KMAX = 32;                   // largest k
static constexpr size_t DTW_EDGE_CAP = 256u << 20;    // bytes of edge arrays per launch
static constexpr size_t DTW_CHUNK_CAP = 64u << 20;    // bytes of distance rows per query chunk
static constexpr int DTW_QCHUNK = 1024;               // queries per chunk at most

#pragma clang fp contract(off)
// One DP row of a strip: cells (r, c0 .. c0 + 31).  prev holds the row above and is replaced by this
// row; diag = D(r-1, c0-1), left = D(r, c0-1).  qs: the padded query's frame c0 (wave-uniform; the
// frames before frame 0 are zeros, so their cells' costs are finite and the cells stay +inf like
// their neighbours).  MODE 0: every cell of the row is admissible for every lane; 1: the band select
// (three more instructions per cell); 2: row 0, the band select and the start cell.
template <int F, int MODE>
__device__ __forceinline__ void dtw_row(double (&prev)[DTW_STRIP], double diag, double left, const double (&bf)[F],
                                        const double *__restrict__ qs, int c0, int r, int w)
{
#pragma unroll
    for (int j = 0; j < DTW_STRIP; j++) {
        const int c = c0 + j;
        const double *qc = qs + j * F;
        double t = bf[0] - qc[0];
        double cost = t * t;
#pragma unroll
        for (int f = 1; f < F; f++) {
            t = bf[f] - qc[f];
            cost = cost + t * t;
        }
        double best = dtw_min(dtw_min(prev[j], left), diag);
        if (MODE == 2 && c == 0) best = 0.0;  // D(0,0) = c(0,0)
        double v = cost + best;
        if (MODE != 0) {
            const int d = r - c;
            v = (d < 0 ? -d : d) <= w ? v : (double)INFINITY;
        }
        diag = prev[j];
        prev[j] = v;
        left = v;
    }
}
#pragma clang fp contract(on)

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
        if (n >= 1 && n <= Tq && mmax > 0) {
            const double *__restrict__ q = apad + (uq * (Tq + DTW_STRIP) + DTW_STRIP) * F;  // frame 0
            const double *__restrict__ br = b + (inr ? ref : 0) * (int64_t)Tr * F;
            const int dl = n > m ? n - m : m - n;
            const int w = window < 0 ? DTW_WBIG : min(max(window, dl), DTW_WBIG);
            const int wmax = wave_max_uniform(m > 0 ? w : 0);
            const int wmin = -wave_max_uniform(m > 0 ? -w : -DTW_WBIG);
            const int S = (n + DTW_STRIP - 1) / DTW_STRIP;
            for (int s = 0; s < S; s++) {
                const int c0 = n - DTW_STRIP * (S - s);  // end-aligned: c0 < 0 only in strip 0
                const int cf = max(c0, 0);
                const int rlo = max(0, cf - wmax), rhi = min(mmax, c0 + DTW_STRIP + wmax);
                if (rlo >= rhi) continue;
                const bool has_left = s > 0, has_right = s < S - 1;
                const double *__restrict__ qs = q + c0 * F;
                double prev[DTW_STRIP];
#pragma unroll
                for (int j = 0; j < DTW_STRIP; j++) prev[j] = INFINITY;
                auto left_of = [&](int r) {  // D(r, c0 - 1) from the strip before, +inf outside the band
                    const int d = r - (c0 - 1);
                    return (has_left && (d < 0 ? -d : d) <= w) ? edge[(size_t)r * 64] : (double)INFINITY;
                };
                double dg = rlo > 0 ? left_of(rlo - 1) : (double)INFINITY;
                double bf[F], left = left_of(rlo);
#pragma unroll
                for (int f = 0; f < F; f++) bf[f] = br[(size_t)rlo * F + f];
                for (int r = rlo; r < rhi; r++) {
                    const int rn = min(r + 1, rhi - 1);  // the next row's loads, issued before this row's cells
                    double bfn[F];
#pragma unroll
                    for (int f = 0; f < F; f++) bfn[f] = br[(size_t)rn * F + f];
                    const double leftn = left_of(rn);
                    const bool full = r > 0 && r - cf <= wmin && c0 + DTW_STRIP - 1 - r <= wmin;
                    if (r == 0)
                        dtw_row<F, 2>(prev, dg, left, bf, qs, c0, r, w);
                    else if (full)
                        dtw_row<F, 0>(prev, dg, left, bf, qs, c0, r, w);
                    else
                        dtw_row<F, 1>(prev, dg, left, bf, qs, c0, r, w);
                    dg = left;
                    if (has_right)
                        edge[(size_t)r * 64] = prev[DTW_STRIP - 1];
                    else if (r == m - 1)
                        res = prev[DTW_STRIP - 1];
                    left = leftn;
#pragma unroll
                    for (int f = 0; f < F; f++) bf[f] = bfn[f];
                }
            }
        }
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
    return Nr >= 0 && Nr <= 0x7fffffff && Nq >= 0 && Tr >= 1 && Tr <= DTW_TMAX && Tq >= 1 && Tq <= DTW_TMAX &&
           F >= 1 && F <= DTW_FMAX;
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
    return ((size_t)dtw_waves(nq, Nr, Tr) * Tr * 64 * 8 + 255) & ~(size_t)255;
}
// the padded copy of one chunk's queries
static size_t dtw_pad_bytes(int64_t nq, int Tq, int F)
{
    return (((size_t)nq * (Tq + DTW_STRIP) * F * 8) + 255) & ~(size_t)255;
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
    const int64_t pad_elems = nq * (Tq + DTW_STRIP) * F;
    hipLaunchKernelGGL(dtw_pad, dim3((unsigned)std::min<int64_t>((pad_elems + 255) / 256, 4096)), dim3(256), 0, s,
                       a_rows, nq, Tq, F, a);
    const dim3 grid((unsigned)G), block(64);
#define DTW_GO(FF)                                                                                                 \
    case FF:                                                                                                       \
        hipLaunchKernelGGL(dtw_dp<FF>, grid, block, 0, s, a, len_a, nq, Tq, b, len_b, Nr, Tr, window, dist, edge); \
        break;
    switch (F) {
        DTW_GO(1) DTW_GO(2) DTW_GO(3) DTW_GO(4) DTW_GO(5) DTW_GO(6) DTW_GO(7) DTW_GO(8)
    default: return DSP_ERR_ARGS;
    }
#undef DTW_GO
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
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
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return DSP_ERR_HIP + (int)e;
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
