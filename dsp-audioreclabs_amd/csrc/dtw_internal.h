// dtw_internal.h -- what dtw.hip (distances, k nearest neighbours) and dtw_align.hip (alignment
// paths, DBA) share: the plan's constants, the wave reduction of the loop bounds and the one-
// instruction minimum.  The kernels themselves stay in their own files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dsp {

static constexpr int DTW_STRIP = 32;                  // DP cells a lane keeps in registers
static constexpr int DTW_TMAX = 1024;                 // longest padded sequence
static constexpr int DTW_FMAX = 8;                    // most feature channels
static constexpr int DTW_WAVES = 4096;                // persistent waves per launch (16 per CU)
static constexpr int DTW_WBIG = 4096;                 // "no band": wider than any grid in the plan

__device__ __forceinline__ int wave_max_uniform(int v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = max(v, __shfl_xor(v, m, 64));
    return __builtin_amdgcn_readfirstlane(v);
}

// min of two values that are never NaN (finite costs and +inf), as the one instruction it is: fmin()
// makes the compiler re-canonicalise every DP value it carries round the row loop (one more
// v_max_f64 x, x per cell on top of the 3F + 2 the cell needs)
__device__ __forceinline__ double dtw_min(double x, double y)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
    return r;
}

}  // namespace dsp
