// dhmm_cells.h -- what the two connected-word decoders share: dhmm_decode.hip (a free loop of the word models,
// DESIGN.md §4.15) and dhmm_grammar.hip (a word-pair grammar, §4.19).  Both keep a lane per word model and the
// NS END-aligned slots of that model in registers (hmm_internal.h: dhmm_decode_pack's layout).
//   decode_cells   one frame of the NS slots of every lane's model, (V, start) replaced in place
//   decode_load    a frame's emissions for every lane, decode_ahead the slots asked for one frame ahead
//   decode_wave_min / decode_readlane / decode_dpp   the 64-lane minimum of the exits
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dtw_internal.h"

namespace dsp {

// a DPP move of both halves of a double; CTRL permutes lanes within a row of 16, every lane has a source
template <int CTRL>
__device__ __forceinline__ double decode_dpp(double x)
{
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double decode_readlane(double x, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}
// the smallest of the 64 lanes' values (never NaN), wave-uniform; +0.0 and -0.0 count as equal here and
// the caller takes the winning lane's own bits
__device__ __forceinline__ double decode_wave_min(double x)
{
    x = dtw_min(x, decode_dpp<0xB1>(x));   // quad_perm [1,0,3,2]
    x = dtw_min(x, decode_dpp<0x4E>(x));   // quad_perm [2,3,0,1]
    x = dtw_min(x, decode_dpp<0x141>(x));  // row_half_mirror: the other quad of the 8
    x = dtw_min(x, decode_dpp<0x140>(x));  // row_mirror: the other 8 of the row
    const double r0 = decode_readlane(x, 0), r1 = decode_readlane(x, 16), r2 = decode_readlane(x, 32),
                 r3 = decode_readlane(x, 48);
    return dtw_min(dtw_min(r0, r1), dtw_min(r2, r3));
}

// slots whose emissions are asked for one frame ahead: all of them up to 16 slots; at 32 the upper 16, which
// the descending sweep needs first -- the lower 16 are asked for when the frame starts and arrive behind the
// upper cells (a second full set of 64 registers would push the cells' operands out of the register file)
constexpr int decode_ahead(int NS) { return NS == 32 ? 16 : NS; }

// One frame of the NS slots of every lane's model: v, st hold frame t-1 and are replaced by frame t.
// eh, el: the frame's emissions, the upper slots (asked for a frame ahead) and the lower ones; trr / ltr: (stay, cost of coming in) per slot in registers or, for NS = 32,
// in LDS at this lane; j0: the lane's entry slot; xprev: what enters there with start t -- the wave's X(t-1)
// in the loop decoder, the lane's own G(t-1, c) under a grammar.
template <int NS>
__device__ __forceinline__ void decode_cells(double (&v)[NS], int (&st)[NS], const double (&eh)[decode_ahead(NS)],
                                             const double (&el)[NS - decode_ahead(NS) + 1],
                                             const double2 (&trr)[NS == 32 ? 1 : NS], const double2 *ltr, int j0,
                                             double xprev, int t)
{
    // inside the body, so that an including file's contraction mode stays what it was
#pragma clang fp contract(off)
    constexpr int LO = NS - decode_ahead(NS);
    // at 32 slots the 32 masks (j == j0) would be kept in 64 scalar registers across the frames and spilled
    // from there; a compare per cell on a value the compiler cannot see through is cheaper
    if constexpr (NS == 32) asm volatile("" : "+v"(j0));
    // slots in descending order: slot j reads frame t-1 of slots j and j-1 only, so it is replaced in place
#pragma unroll
    for (int j = NS - 1; j >= 0; j--) {
        double2 sa;
        if constexpr (NS == 32)
            sa = ltr[j * 64];
        else
            sa = trr[j];
        const bool ent = j == j0;
        const double pv = ent ? xprev : (j > 0 ? v[j > 0 ? j - 1 : 0] : (double)INFINITY);
        const int ps = ent ? t : (j > 0 ? st[j > 0 ? j - 1 : 0] : -1);
        const double a = v[j] + sa.x;
        const double b = pv + sa.y;
        const bool advance = b < a;
        v[j] = (j >= LO ? eh[j >= LO ? j - LO : 0] : el[j < LO ? j : 0]) + (advance ? b : a);
        st[j] = advance ? ps : st[j];
    }
}

// CNT slots from slot J0 on of symbol k for every lane, the highest first; k is clamped into the table
template <int NS, int J0, int CNT, int LEN>
__device__ __forceinline__ void decode_load(double (&e)[LEN], const double *__restrict__ tabl, int k, int K)
{
    const double *__restrict__ row = tabl + (size_t)min((unsigned)k, (unsigned)(K - 1)) * (NS * 64);
#pragma unroll
    for (int j = CNT - 1; j >= 0; j--) e[j] = row[(J0 + j) * 64];
}

}  // namespace dsp
