// zscore.hip -- z-score (src/feature_extraction.py:157-181), numpy axis-0 order, for gfx950.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsp_audiorec.h"

namespace dsp {

#pragma clang fp contract(off)
// numpy's axis-0 sums are sequential in row order per column, so each column is one dependent
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
    hipLaunchKernelGGL(dsp::zscore_fit_kernel, dim3((unsigned)((D + dsp::ZS_C - 1) / dsp::ZS_C)), dim3(dsp::ZS_T), 0,
                       (hipStream_t)stream, X, N, D, mean, std);
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
