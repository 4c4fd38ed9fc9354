// dtw_internal.h -- what dtw.hip (distances, k nearest neighbours) and dtw_align.hip (alignment
// paths, DBA) share: the plan's constants and host arithmetic, the F dispatch, and the dynamic
// programme itself -- the row body dtw_row and the sweep of one tile's strips, dtw_sweep.  hmm.hip
// takes the plan, the dispatch and the small helpers from here too (csr_pairs.h: the pair list).
//
// The sweep.  A wave owns a tile: ONE sequence of the uniform side (length n) against 64 sequences of
// the lanes' side, lane l owning the pair (uniform, its own sequence of length m).  The uniform
// sequence's frames are the same for every lane, so they are read with wave-uniform addresses
// (scalar loads, no LDS and no vector-memory traffic per cell), and only the lane's own frame -- F
// values per DP row -- comes through the vector path, prefetched one row ahead.  The lane keeps a
// strip of 32 DP cells (32 consecutive uniform frames) in registers and sweeps its own sequence's
// frames in the outer loop, the strip loop fully unrolled so the register array is never indexed
// at run time.  Strips are END-aligned (the last one ends at uniform frame n - 1, the first may
// start before frame 0 with those cells held at +inf), so the strip's last register is both the
// edge handed to the next strip and, in the last strip, the result; dtw_pad (dtw.hip) first copies
// the uniform sequences behind 32 frames of zeros, so those reads stay inside the copy's row and
// every strip reads its 32 uniform frames at constant offsets from one base.  A strip hands its edge
// column D(., last) to the next one through a per-wave array in the workspace laid out [row][lane]
// (coalesced); the first strip reads +inf, the last writes nothing.
// Loop bounds are wave-uniform (the largest length and band of the wave's lanes); rows past a
// lane's own length compute values nothing reads.  Rows of a strip that are admissible for no lane
// are skipped; a row that is admissible in all its 32 cells for every lane runs a body without the
// band select (row 0, with the start cell, has a body of its own).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsp_audiorec.h"

namespace dsp {

static constexpr int DTW_STRIP = 32;                  // DP cells a lane keeps in registers
static constexpr int DTW_TMAX = 1024;                 // longest padded sequence
static constexpr int DTW_FMAX = 8;                    // most feature channels
static constexpr int DTW_WAVES = 4096;                // persistent waves per launch (16 per CU)
static constexpr int DTW_WBIG = 4096;                 // "no band": wider than any grid in the plan

// ---- host arithmetic ----
static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
static inline bool dtw_shape_in_plan(int Ta, int Tb, int F)
{
    return Ta >= 1 && Ta <= DTW_TMAX && Tb >= 1 && Tb <= DTW_TMAX && F >= 1 && F <= DTW_FMAX;
}
// the padded copy of rows sequences [rows, T + DTW_STRIP, F] (dtw_pad)
static inline size_t dtw_pad_bytes(int64_t rows, int T, int F)
{
    return up256((size_t)rows * (T + DTW_STRIP) * F * 8);
}
// out [rows, T + DTW_STRIP, F]: DTW_STRIP frames of zeros before each sequence of in [rows, T, F] (dtw.hip)
void dtw_launch_pad(hipStream_t s, const double *in, int64_t rows, int T, int F, double *out);
// what an entry point returns after its launches
static inline int dtw_launch_status()
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
}

// launches KERNEL<F> for the plan's F = 1 .. 8; the arguments after KERNEL are hipLaunchKernelGGL's
#define DTW_CASE_F(FF, KERNEL, ...)                   \
    case FF:                                          \
        hipLaunchKernelGGL(KERNEL<FF>, __VA_ARGS__); \
        break;
#define DTW_LAUNCH_F(F, KERNEL, ...)                                                                      \
    switch (F) {                                                                                          \
        DTW_CASE_F(1, KERNEL, __VA_ARGS__) DTW_CASE_F(2, KERNEL, __VA_ARGS__) DTW_CASE_F(3, KERNEL, __VA_ARGS__) \
        DTW_CASE_F(4, KERNEL, __VA_ARGS__) DTW_CASE_F(5, KERNEL, __VA_ARGS__) DTW_CASE_F(6, KERNEL, __VA_ARGS__) \
        DTW_CASE_F(7, KERNEL, __VA_ARGS__) DTW_CASE_F(8, KERNEL, __VA_ARGS__)                             \
    default: return DSP_ERR_ARGS;                                                                         \
    }

// ---- device side ----
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

#pragma clang fp contract(off)
// One DP row of a strip: cells (r, c0 .. c0 + 31), r the lane's frame, c the uniform frame.  prev
// holds the row above and is replaced by this row; diag = D(r-1, c0-1), left = D(r, c0-1).  qs: the
// padded uniform sequence's frame c0 (the frames before frame 0 are zeros, so their cells' costs
// are finite and the cells stay +inf like their neighbours).  MODE 0: every cell of the row is
// admissible for every lane; 1: the band select (three more instructions per cell); 2: row 0, the
// band select and the start cell.
// DIR: the predecessor codes as well.  w0 collects "the diagonal equals the minimum", w1 "left does",
// one bit per cell, cell 31 in bit 0; without DIR w0 and w1 are left alone.
template <int F, int MODE, bool DIR>
__device__ __forceinline__ void dtw_row(double (&prev)[DTW_STRIP], double diag, double left, const double (&bf)[F],
                                        const double *__restrict__ qs, int c0, int r, int w, uint32_t &w0,
                                        uint32_t &w1)
{
    uint32_t md = 0, ml = 0;
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
        // m = 2 m + (x == best): each compare's bit is shifted in through the carry, two instructions
        // per bit (a select and an or of a constant per bit are three)
        if (DIR)
            asm("v_cmp_eq_f64 vcc, %2, %4\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc\n\t"
                "v_cmp_eq_f64 vcc, %3, %4\n\tv_addc_co_u32 %1, vcc, %1, %1, vcc"
                : "+v"(md), "+v"(ml)
                : "v"(diag), "v"(left), "v"(best)
                : "vcc");
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
    if (DIR) {
        w0 = md;
        w1 = ml;
    }
}

// All strips of one tile (above): D(n-1, m-1) of the lane's pair before the sqrt, +inf where m == 0.
// q: frame 0 of the padded uniform sequence, 1 <= n <= its width; br: the lane's own sequence, m
// its length or 0 (nothing of such a lane is used), mmax > 0 the wave's largest m.  edge: this
// wave's edge column at this lane, [row][lane]; only sequences longer than one strip use it.
// DIR: each row's codes go to dir, this wave's words at this lane, [strip][row][lane] with Tl rows
// per strip (the lanes' padded width), w1 in the high half; dir == NULL: not stored.
template <int F, bool DIR>
__device__ __forceinline__ double dtw_sweep(const double *__restrict__ q, const double *__restrict__ br, int n, int m,
                                            int mmax, int window, int Tl, double *__restrict__ edge,
                                            unsigned long long *dir)
{
    double res = INFINITY;
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
        unsigned long long *drow = DIR ? dir + (size_t)s * (size_t)Tl * 64 : nullptr;
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
            uint32_t w0, w1;
            if (r == 0)
                dtw_row<F, 2, DIR>(prev, dg, left, bf, qs, c0, r, w, w0, w1);
            else if (full)
                dtw_row<F, 0, DIR>(prev, dg, left, bf, qs, c0, r, w, w0, w1);
            else
                dtw_row<F, 1, DIR>(prev, dg, left, bf, qs, c0, r, w, w0, w1);
            dg = left;
            if (DIR && dir) drow[(size_t)r * 64] = ((unsigned long long)w1 << 32) | w0;
            if (has_right)
                edge[(size_t)r * 64] = prev[DTW_STRIP - 1];
            else if (r == m - 1)
                res = prev[DTW_STRIP - 1];
            left = leftn;
#pragma unroll
            for (int f = 0; f < F; f++) bf[f] = bfn[f];
        }
    }
    return res;
}
#pragma clang fp contract(on)

}  // namespace dsp
