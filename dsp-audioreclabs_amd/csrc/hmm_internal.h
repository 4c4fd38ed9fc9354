// hmm_internal.h -- what the left-to-right HMM files share: hmm.hip (Gaussian), dhmm.hip (discrete, Viterbi),
// dhmm_fb.hip (discrete, forward-backward), dhmm_decode.hip and dhmm_grammar.hip (connected words, free loop and
// word-pair grammar; their cell sweep is dhmm_cells.h) and dhmm_force.hip (forced alignment).
//   bounds         of a model set and of a launch, and the discrete plan's dhmm_in_plan
//   seg rows       hmm_walk_back (the lane's path from the direction words), hmm_seg_ok (a given row's check)
//   the record     of a discrete model: dhmm_record / dhmm_pitch / dhmm_tr_offset / dhmm_lds_bytes, dhmm_pack
//                  (the set into the workspace), dhmm_stage (one record into LDS), dhmm_lds_limit
//   dhmm_with_slots    the 8 / 16 / 32 register-slot dispatch of a launch
//   the set by model   dhmm_decode_pack with its plan and launch: the layout a wave reads whose lanes are models
//                  (dhmm_decode.hip) or transcript positions (dhmm_force.hip)
// Kernels are static, as in csr_pairs.h: every object that launches one has its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dtw_internal.h"

namespace dsp {

static constexpr int HMM_SMAX = 32;           // states a lane keeps in registers at most
static constexpr int64_t HMM_CMAX = 1 << 20;  // models in a set at most
static constexpr int HMM_GCHUNK = 1024;       // models per launch at most
static constexpr int HMM_BATCH = 16;          // members whose loads a thread of an ordered sum keeps in flight
static constexpr int DHMM_SMAX = HMM_SMAX;
static constexpr int DHMM_KMAX = 256;               // symbols of the alphabet at most
static constexpr size_t DHMM_GP_CAP = 256u << 20;   // bytes of per-pair tables G_p per pair chunk (dhmm_fb.hip)

// register slots of a launch: the smallest of 8, 16, 32 that holds Smax
static inline int dhmm_slots(int Smax) { return Smax <= 8 ? 8 : (Smax <= 16 ? 16 : 32); }

// f(std::integral_constant<int, NS>()) for NS = 8, 16 or 32: a launch's slots as a template argument
template <class F>
static inline auto dhmm_with_slots(int NS, F f)
{
    if (NS == 8) return f(std::integral_constant<int, 8>());
    if (NS == 16) return f(std::integral_constant<int, 16>());
    return f(std::integral_constant<int, 32>());
}

static inline bool dhmm_in_plan(int64_t C, int64_t N, int64_t P, int T, int Smax, int K)
{
    return C >= 0 && C <= HMM_CMAX && N >= 0 && N < 0x7fffffff && P >= 0 && P < 0x7fffffff && Smax >= 1 &&
           Smax <= DHMM_SMAX && K >= 1 && K <= DHMM_KMAX && T >= 1 && T <= DTW_TMAX;
}

// ---- seg rows ----
// bytes of direction words a persistent wave owns in the workspace: a 32-bit word per row and lane
static inline size_t hmm_dir_bytes(int T) { return (size_t)T * 64 * 4; }

// The lane's own walk back through its direction words dir [row][lane] (n rows, S states; state s is slot
// s + slots - S, that bit of a row's word) into the seg row ps [Smax]: the first frame of each state, -1 behind
// the S states, and -1 everywhere when !res_ok (the pair's score is +inf).  At most n - 1 steps and the row only
// decreases, so the walk ends inside the pair's words whatever the bits hold.
__device__ __forceinline__ void hmm_walk_back(const uint32_t *dir, int n, int S, int slots, int Smax, bool res_ok,
                                              int32_t *__restrict__ ps)
{
    int filled = 0;
    if (res_ok) {
        int s = S - 1;
        for (int r = n - 1; r >= 1 && s > 0; r--)
            if ((dir[(size_t)r * 64] >> (s + slots - S)) & 1) ps[s--] = r;
        for (; s > 0; s--) ps[s] = s;  // not reached with the sweep's own words
        ps[0] = 0;
        filled = S;
    }
    for (int i = filled; i < Smax; i++) ps[i] = -1;
}

// a given seg row is well formed for a model of S states and a sequence of n frames: ps[0] = 0, strictly
// increasing over the S states, ps[S-1] < n
__device__ __forceinline__ bool hmm_seg_ok(const int32_t *__restrict__ ps, int S, int n)
{
    bool ok = ps[0] == 0;
    for (int s = 0; ok && s < S; s++) {
        const int b = ps[s], e = s + 1 < S ? ps[s + 1] : n;
        ok = b >= 0 && b < e && e <= n;
    }
    return ok;
}

// ---- the record of a discrete model ----
// In the workspace: the table transposed to [K][NS] doubles -- one symbol's slots contiguous -- then (stay,
// adv[s-1]) per slot, END-aligned to the NS slots: state s of a model of S states sits in slot s + NS - S, so
// the result is always slot NS - 1; the leading slots hold 0.0 (cells that start at +inf, or at probability 0,
// and stay there).  In LDS: symbol k's slots at byte k * dhmm_pitch(NS), the 16 bytes of padding making the pitch
// an odd number of 16-byte units (NS is a multiple of 4), so symbols k and k' share a bank window only when
// k = k' (mod 16) -- and then broadcast if k = k'; the transitions behind the table.
__host__ __device__ constexpr size_t dhmm_record(int K, int NS) { return (size_t)K * NS + 2 * (size_t)NS; }  // doubles
__host__ __device__ constexpr int dhmm_pitch(int NS) { return NS * 8 + 16; }
__host__ __device__ constexpr size_t dhmm_tr_offset(int K, int NS) { return (size_t)K * dhmm_pitch(NS); }
__host__ __device__ constexpr size_t dhmm_lds_bytes(int K, int NS) { return dhmm_tr_offset(K, NS) + (size_t)NS * 16; }

// rec [C][dhmm_record(K, NS)]; a model with an invalid n_states gets zeros (never read)
static __global__ __launch_bounds__(256) void dhmm_pack(const double *__restrict__ emit, const double *__restrict__ stay,
                                                        const double *__restrict__ adv, const int32_t *__restrict__ n_states,
                                                        int64_t C, int Smax, int K, int NS, double *__restrict__ rec)
{
    const int64_t R = (int64_t)dhmm_record(K, NS), total = C * R;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t c = e / R;
        const int r = (int)(e % R);
        const bool tab = r < K * NS;
        const int j = tab ? r % NS : (r - K * NS) / 2;
        const int S = n_states[c], s = j - (NS - S);
        double v = 0.0;
        if (S >= 1 && S <= Smax && s >= 0) {
            const int64_t cs = c * Smax + s;
            if (tab)
                v = emit[cs * K + r / NS];
            else if ((r - K * NS) % 2 == 0)
                v = stay[cs];
            else
                v = s > 0 ? adv[cs - 1] : 0.0;
        }
        rec[e] = v;
    }
}

// one model's record rec into the wave's LDS, in 16-byte pieces: K * NS / 2 of the table, then NS of the
// transitions, which lie where the slots of a symbol K would
template <int NS>
__device__ __forceinline__ void dhmm_stage(unsigned char *lds, const double *__restrict__ rec, int K, int lane)
{
    const double2 *__restrict__ src = (const double2 *)rec;
    const int ne = K * (NS / 2);
    __syncthreads();  // one wave: the reads of the table staged before are done
    for (int i = lane; i < ne + NS; i += 64) {
        const int row = i < ne ? i / (NS / 2) : K, piece = i < ne ? i % (NS / 2) : i - ne;
        *(double2 *)(lds + (size_t)row * dhmm_pitch(NS) + (size_t)piece * 16) = src[i];
    }
    __syncthreads();
}

// K = 256 at 32 slots is past the default limit of a kernel's dynamic LDS
template <class Kernel>
static inline hipError_t dhmm_lds_limit(Kernel kernel, size_t lds)
{
    if (lds <= 65536) return hipSuccess;
    return hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// ---- the set for a wave whose lanes read it by model (dhmm_decode.hip: a lane per model; dhmm_force.hip: a
// lane per transcript position, reading its word's column) ----
// tab [K][NS][64] doubles, END-aligned like the record above (state s of a model of S states in slot s + NS - S,
// so every model's exit is slot NS - 1); the slots before a model's first state, a model with an invalid
// n_states and the columns c >= C hold +inf, so their cells start at +inf and stay there.  tr [NS][64] pairs
// (stay, cost of coming in from the slot before): adv[s-1], and at the model's first slot enter[c] (NULL: 0.0).
// j0 [64]: that first slot, NS where the model is never entered.
struct DecodePlan {
    int NS;
    size_t tab, tr, j0;  // bytes of the three parts
    size_t total() const { return tab + tr + j0; }
};
static inline DecodePlan decode_plan(int Smax, int K)
{
    DecodePlan pl;
    pl.NS = dhmm_slots(Smax);
    pl.tab = up256((size_t)K * pl.NS * 64 * 8);
    pl.tr = up256((size_t)pl.NS * 64 * 16);
    pl.j0 = up256(64 * 4);
    return pl;
}

static __global__ __launch_bounds__(256) void dhmm_decode_pack(const double *__restrict__ emit, const double *__restrict__ stay,
                                                               const double *__restrict__ adv, const int32_t *__restrict__ n_states,
                                                               const double *__restrict__ enter, int C, int Smax, int K, int NS,
                                                               double *__restrict__ tab, double2 *__restrict__ tr,
                                                               int32_t *__restrict__ j0)
{
    const int ntab = K * NS * 64, ntr = NS * 64;
    for (int e = (int)blockIdx.x * 256 + (int)threadIdx.x; e < ntab + ntr + 64; e += (int)gridDim.x * 256) {
        const int c = e % 64;
        const int S = c < C ? n_states[c] : 0;
        const bool ok = S >= 1 && S <= Smax;
        if (e >= ntab + ntr) {
            j0[c] = ok ? NS - S : NS;
            continue;
        }
        const int j = (e / 64) % NS, s = ok ? j - (NS - S) : -1;
        const bool in = s >= 0;
        const int64_t cs = (int64_t)c * Smax + s;
        if (e < ntab) {
            tab[e] = in ? emit[cs * K + e / (NS * 64)] : (double)INFINITY;
        } else {
            double2 v = make_double2(0.0, 0.0);
            if (in) {
                v.x = stay[cs];
                v.y = s > 0 ? adv[cs - 1] : (enter ? enter[c] : 0.0);
            }
            tr[e - ntab] = v;
        }
    }
}
// the pack's launch on stream s into the plan's three parts at ws
static inline void dhmm_decode_pack_launch(hipStream_t s, const DecodePlan &pl, void *ws, const double *emit, const double *stay,
                                           const double *adv, const int32_t *n_states, const double *enter, int C, int Smax,
                                           int K)
{
    const int64_t elems = (int64_t)K * pl.NS * 64 + pl.NS * 64 + 64;
    hipLaunchKernelGGL(dhmm_decode_pack, dim3((unsigned)((elems + 255) / 256 < 1024 ? (elems + 255) / 256 : 1024)), dim3(256), 0, s,
                       emit, stay, adv, n_states, enter, C, Smax, K, pl.NS, (double *)ws, (double2 *)((char *)ws + pl.tab),
                       (int32_t *)((char *)ws + pl.tab + pl.tr));
}

}  // namespace dsp
