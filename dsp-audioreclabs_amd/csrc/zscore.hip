// zscore.hip -- z-score (src/feature_extraction.py:157-181), numpy axis-0 order, for gfx950:
// D >= 2 columns sequential over the rows (zscore_fit_kernel), D = 1 numpy's pairwise sum of the
// one contiguous column (zscore_fit1_kernel).  C-contiguous rows; bit for bit np.mean / np.std.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsp_audiorec.h"

namespace dsp {

#pragma clang fp contract(off)
// D >= 2: numpy's axis-0 sums are sequential in row order per column, so each column is one dependent
// chain of fp64 adds; the kernel's job is to keep that chain fed.  One workgroup per ZS_C columns:
// waves 1-3 stage the next ZS_R-row tile of those columns in LDS (coalesced when the row is
// narrower than ZS_C) while lane c of wave 0 adds the current tile's column c in row order from
// LDS (reads issued ahead of the adds), then a barrier swaps the buffers.  Pass 0 sums x, pass 1
// (x - mean)^2.  Round 5 ran one thread per column with a dependent global load per row (46 ms
// for 100 000 x 15); one wave per column with lane_read 7.8 ms (v_readlane latency per add).
static constexpr int ZS_T = 256, ZS_R = 256, ZS_C = 16;
__global__ __launch_bounds__(ZS_T) void zscore_fit_kernel(const double *X, int64_t N, int D, double *mean, double *std)
{
    __shared__ double tile[2][ZS_R * ZS_C];
    const int c0 = (int)blockIdx.x * ZS_C, nc = min(ZS_C, D - c0), tid = threadIdx.x;
    const int64_t ntile = (N + ZS_R - 1) / ZS_R;
    // waves 1-3: rows [t ZS_R, +ZS_R) x columns [c0, c0 + nc), every load of the tile issued
    // before the first LDS store (a store waits for its load: one at a time, a tile cost ~7 us)
    constexpr int LPT = (ZS_R * ZS_C + ZS_T - 64 - 1) / (ZS_T - 64);
    auto load = [&](int64_t t, int buf) {
        double v[LPT];
#pragma unroll
        for (int u = 0; u < LPT; u++) {
            const int e = tid - 64 + u * (ZS_T - 64);
            const int r = e / nc, c = e - r * nc;
            const int64_t row = t * ZS_R + r;
            v[u] = (e < ZS_R * nc && row < N) ? X[row * D + c0 + c] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < LPT; u++) {
            const int e = tid - 64 + u * (ZS_T - 64);
            const int r = e / nc, c = e - r * nc;
            if (e < ZS_R * nc) tile[buf][r * ZS_C + c] = v[u];
        }
    };
    double m = 0.0, acc = 0.0;
    for (int pass = 0; pass < 2; pass++) {
        acc = 0.0;
        if (tid >= 64) load(0, 0);
        __syncthreads();
        for (int64_t t = 0; t < ntile; t++) {
            const int buf = (int)(t & 1);
            if (tid >= 64) {
                if (t + 1 < ntile) load(t + 1, buf ^ 1);
            } else if (tid < nc) {
                const int rows = (int)min((int64_t)ZS_R, N - t * ZS_R);
                const double *col = tile[buf] + tid;
                // batches of 16 rows: 16 LDS reads, then 16 adds (each waits only for its own read).
                // Reading the next batch before this batch's adds measured slower: 16 ahead 4.16
                // ms, 8 ahead 4.22 ms, against 2.69 ms (100 000 x 15, profiles/r06i/j/z)
                int r = 0;
                for (; r + 16 <= rows; r += 16) {
                    double v[16];
#pragma unroll
                    for (int u = 0; u < 16; u++) v[u] = col[(r + u) * ZS_C];
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        if (pass == 0) {
                            acc = acc + v[u];
                        } else {
                            const double x = v[u] - m;
                            acc = acc + x * x;
                        }
                    }
                }
                for (; r < rows; r++) {
                    if (pass == 0) {
                        acc = acc + col[r * ZS_C];
                    } else {
                        const double x = col[r * ZS_C] - m;
                        acc = acc + x * x;
                    }
                }
            }
            __syncthreads();
        }
        if (pass == 0) m = acc / (double)N;
    }
    if (tid < nc) {
        const double sd = sqrt(acc / (double)N);
        mean[c0 + tid] = m;
        std[c0 + tid] = sd == 0.0 ? 1.0 : sd;
    }
}

// D = 1.  numpy coalesces the two axes of a C-contiguous (N, 1) array, so its axis-0 reduction is
// the reduction of one contiguous run, which numpy sums in chunks of 8192 elements (its buffer),
// the chunks' sums added to the total in order, and each chunk pairwise, not in row order:
//   sum(a, n) = a[0] + ... + a[n-1] in order                                   for n < 8,
//             = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 tail in order,
//               r_j the running sum of a[j], a[j + 8], ...                      for n <= 128,
//             = sum(a, h) + sum(a + h, n - h), h = n / 2 rounded down to a multiple of 8, otherwise.
// The std applies the same sum to (x - mean)^2.  This shape is no hot path (the recogniser has 15
// columns), so the kernel is built to be right: one workgroup; thread 0 walks the chunks and each
// chunk's recursion with an explicit stack and hands out its next ZS1_T leaf blocks (n <= 128),
// one thread sums each block, and thread 0 folds the block sums in numpy's order on a value stack
// -- after a block, one addition for every split, and every chunk, that this block completes.
static constexpr int ZS1_T = 256, ZS1_CHUNK = 8192, ZS1_STACK = 32;  // two entries per level, 7 levels
__device__ __forceinline__ double zs1_term(const double *X, int64_t i, int pass, double m)
{
    const double v = X[i];
    if (pass == 0) return v;
    const double x = v - m;
    return x * x;
}
__device__ __forceinline__ double zs1_block(const double *X, int64_t off, int n, int pass, double m)
{
    double res = 0.0;
    if (n < 8) {
        for (int i = 0; i < n; i++) res = res + zs1_term(X, off + i, pass, m);
        return res;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = zs1_term(X, off + j, pass, m);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] = r[j] + zs1_term(X, off + i + j, pass, m);
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res = res + zs1_term(X, off + i, pass, m);
    return res;
}
__global__ __launch_bounds__(ZS1_T) void zscore_fit1_kernel(const double *X, int64_t N, double *mean, double *std)
{
    __shared__ int64_t node_off[ZS1_STACK], node_n[ZS1_STACK];  // pending subtrees; n < 0: "add the two on top"
    __shared__ double vstack[ZS1_STACK];
    __shared__ int64_t blk_off[ZS1_T];
    __shared__ int blk_n[ZS1_T], blk_adds[ZS1_T];
    __shared__ double blk_sum[ZS1_T];
    __shared__ int nblk_s;
    __shared__ double m_s;
    const int tid = threadIdx.x;
    double m = 0.0;
    for (int pass = 0; pass < 2; pass++) {
        int sp = 0, vsp = 1;  // thread 0's stack pointers; vstack[0] is the running total
        int64_t next = 0;     // the first row of the next chunk
        if (tid == 0) vstack[0] = 0.0;
        for (;;) {
            if (tid == 0) {
                // the next blocks in order; a batch never ends in front of a pending addition
                int nb = 0;
                while (sp > 0 ? (nb < ZS1_T || node_n[sp - 1] < 0) : (nb < ZS1_T && next < N)) {
                    if (sp == 0) {  // a new chunk: its sum, then total + sum
                        node_n[sp++] = -1;
                        node_off[sp] = next;
                        node_n[sp++] = min((int64_t)ZS1_CHUNK, N - next);
                        next += ZS1_CHUNK;
                    }
                    sp--;
                    const int64_t off = node_off[sp], n = node_n[sp];
                    if (n < 0) {
                        blk_adds[nb - 1]++;
                    } else if (n <= 128) {
                        blk_off[nb] = off;
                        blk_n[nb] = (int)n;
                        blk_adds[nb] = 0;
                        nb++;
                    } else {
                        int64_t h = n / 2;
                        h -= h % 8;
                        node_n[sp++] = -1;
                        node_off[sp] = off + h;
                        node_n[sp++] = n - h;
                        node_off[sp] = off;
                        node_n[sp++] = h;
                    }
                }
                nblk_s = nb;
            }
            __syncthreads();
            const int nb = nblk_s;
            if (nb == 0) break;  // the whole workgroup: the recursion is done
            if (tid < nb) blk_sum[tid] = zs1_block(X, blk_off[tid], blk_n[tid], pass, m);
            __syncthreads();
            if (tid == 0)
                for (int i = 0; i < nb; i++) {
                    vstack[vsp++] = blk_sum[i];
                    for (int a = 0; a < blk_adds[i]; a++) {
                        const double hi = vstack[--vsp], lo = vstack[--vsp];
                        vstack[vsp++] = lo + hi;
                    }
                }
        }
        if (pass == 0) {
            if (tid == 0) m_s = vstack[0] / (double)N;
            __syncthreads();
            m = m_s;
        }
    }
    if (tid == 0) {
        const double sd = sqrt(vstack[0] / (double)N);
        mean[0] = m;
        std[0] = sd == 0.0 ? 1.0 : sd;
    }
}

__global__ void zscore_apply_kernel(const double *X, int64_t N, int D, const double *mean,
                                    const double *std, double *out)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N * D) return;
    const int c = (int)(e % D);
    out[e] = (X[e] - mean[c]) / std[c];
}
#pragma clang fp contract(on)

}  // namespace dsp

extern "C" int dsp_zscore_fit(const double *X, int64_t N, int D, double *mean, double *std,
                              void *stream)
{
    if (!X || !mean || !std || N < 1 || D < 1) return DSP_ERR_ARGS;
    if (D == 1)  // one column: numpy's pairwise order (zscore_fit1_kernel)
        hipLaunchKernelGGL(dsp::zscore_fit1_kernel, dim3(1), dim3(dsp::ZS1_T), 0, (hipStream_t)stream, X, N, mean, std);
    else
        hipLaunchKernelGGL(dsp::zscore_fit_kernel, dim3((unsigned)((D + dsp::ZS_C - 1) / dsp::ZS_C)), dim3(dsp::ZS_T),
                           0, (hipStream_t)stream, X, N, D, mean, std);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
}

extern "C" int dsp_zscore_apply(const double *X, int64_t N, int D, const double *mean,
                                const double *std, double *out, void *stream)
{
    if (!X || !mean || !std || !out || N < 0 || D < 1) return DSP_ERR_ARGS;
    if (N == 0) return DSP_OK;
    const int64_t tot = N * D;
    hipLaunchKernelGGL(dsp::zscore_apply_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, X, N, D, mean, std, out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
}
