// csr_pairs.h -- what dtw_align.hip (alignment paths, DBA), hmm.hip (Viterbi paths, re-estimation) and
// vq.hip (nearest codewords, Lloyd re-estimation) do with a CSR pair list (group_start [groups + 1], members [P]: group c against the sequences
// members[p], p in [group_start[c], group_start[c+1])):
//   csr_walk         the tiles of a launch's groups dealt to its persistent waves, a lane per pair
//   csr_group_of     the group that holds a pair
//   csr_waves        the persistent waves of a launch
//   csr_zero, csr_grid   the host side of the chunked re-estimations
//   csr_label        the label of a score matrix [N, C] (hmm.hip, vq.hip)
#pragma once
#include <algorithm>

#include "dtw_internal.h"

namespace dsp {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// A lane's pair of one tile: p the pair (inr: inside its group; outputs are written for those only),
// row the lane's sequence (0 where the pair has none), len its length (0: nothing of the lane is used;
// a member outside [0, N) or a length outside 1 .. T), lmax the largest len of the tile (wave-uniform).
struct CsrLane {
    int64_t p;
    bool inr;
    int row, len, lmax;
};

// Wave wv of G takes the tiles wv, wv + G, ... of the groups cg = 0 .. nc-1, a tile being 64 consecutive
// pairs of ONE group, counted by walking group_start (wave-uniform: scalar loads): group cg has its
// list's pairs inside the window [p_lo, p_hi), pair p being sequence members[p].  group_start == NULL:
// every group has the pairs [p_lo, p_hi) and pair p is sequence p.  len [N] are the sequences' lengths, T
// their padded width.  tile(cg, lane) runs once per tile with every lane of the wave active.
template <class Tile>
__device__ __forceinline__ void csr_walk(int G, int wv, int nc, const int32_t *__restrict__ group_start, int p_lo,
                                         int p_hi, const int32_t *__restrict__ members,
                                         const int32_t *__restrict__ len, int64_t N, int T, Tile tile)
{
    const int lane = (int)threadIdx.x;
    int base = 0;  // tiles of the groups before cg, modulo G
    for (int cg = 0; cg < nc; cg++) {
        const int g0 = group_start ? clampi(group_start[cg], p_lo, p_hi) : p_lo;
        const int g1 = group_start ? clampi(group_start[cg + 1], p_lo, p_hi) : p_hi;
        if (g1 <= g0) continue;
        const int nt = (int)(((int64_t)g1 - g0 + 63) / 64);
        int t0 = wv - base;
        if (t0 < 0) t0 += G;
        base = (int)(((int64_t)base + nt) % G);
        for (int t = t0; t < nt; t += G) {
            CsrLane ln;
            ln.p = (int64_t)g0 + (int64_t)t * 64 + lane;
            ln.inr = ln.p < g1;
            const int ref = ln.inr ? (group_start ? members[ln.p] : (int)ln.p) : -1;
            const bool rok = ref >= 0 && ref < N;
            ln.row = rok ? ref : 0;
            ln.len = rok ? len[ref] : 0;
            if (ln.len < 1 || ln.len > T) ln.len = 0;
            ln.lmax = wave_max_uniform(ln.len);
            tile(cg, ln);
        }
    }
}

// the group that holds pair p: the last c of 0 .. C-1 with group_start[c] <= p (0 when there is none)
__device__ __forceinline__ int64_t csr_group_of(const int32_t *__restrict__ group_start, int64_t C, int64_t p)
{
    int64_t lo = 0, hi = C;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) / 2;
        if (group_start[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// a [na] and b [nb] to zeros before the first pair chunk of a re-estimation.  A kernel, not a memset: the call
// stays a chain of kernel launches, which is what a captured single-stream graph of it replays in order.
template <class A, class B>
static __global__ __launch_bounds__(256) void csr_zero(A *__restrict__ a, int64_t na, B *__restrict__ b, int64_t nb)
{
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < na + nb; e += (int64_t)gridDim.x * 256) {
        if (e < na)
            a[e] = A(0);
        else
            b[e - na] = B(0);
    }
}

// label [N]: the column of the smallest score [N, C] (never NaN) per row, ties to the smaller index, -1
// when every score is +inf
static __global__ __launch_bounds__(256) void csr_label(const double *__restrict__ score, int64_t N, int64_t C,
                                                        int32_t *__restrict__ label)
{
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < N; r += (int64_t)gridDim.x * 256) {
        double best = INFINITY;
        int32_t arg = -1;
        for (int64_t c = 0; c < C; c++) {
            const double v = score[r * C + c];
            if (v < best) {
                best = v;
                arg = (int32_t)c;
            }
        }
        label[r] = arg;
    }
}

// The persistent waves of a launch of tiles tiles: at most DTW_WAVES, and where every wave owns bytes_per_wave
// bytes of the workspace (0: none) no more than CSR_WAVE_CAP holds
static constexpr size_t CSR_WAVE_CAP = 256u << 20;
static inline int csr_waves(int64_t tiles, size_t bytes_per_wave)
{
    const int64_t cap = bytes_per_wave ? std::max<int64_t>(1, (int64_t)(CSR_WAVE_CAP / bytes_per_wave)) : DTW_WAVES;
    return (int)std::max<int64_t>(1, std::min<int64_t>(tiles, std::min<int64_t>(DTW_WAVES, cap)));
}

// blocks of 256 threads striding over elems elements
static inline dim3 csr_grid(int64_t elems)
{
    return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((elems + 255) / 256, 65536)));
}

}  // namespace dsp
