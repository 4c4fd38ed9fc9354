// dhmm_force.hip -- forced alignment of connected utterances against their transcripts, and the embedded
// Viterbi re-estimate from those alignments, over the word models of a discrete-HMM set (dhmm.hip), on gfx950
// (include/dsp_audiorec.h: dsp_dhmm_force_align, dsp_dhmm_force_accumulate).  An extension
// like §4.8-§4.16: nothing here restates a reference file.  Every value is defined bit for bit: the device
// sees only fp64 add and compare and integer counts.
//
// Inputs.  The model set and enter float64 [C] of dsp_dhmm_decode with the same value rules (enter NULL: all
// 0.0); 1 <= C <= 64, Smax <= 32, K <= 256; sym int32 [N, T], len int32 [N], T <= 1024.  trans int32 [N, Wmax]:
// the model of each word of utterance u's transcript in time order, n_trans int32 [N] its word count,
// 1 <= Wmax <= 64; entries of trans behind n_trans[u] are never read through.
// Recurrence.  Utterance u of n frames, transcript w_0 .. w_{L-1}, S_i = n_states[w_i]; position i has the
// states (i, 0 .. S_i - 1); V(-1, ., .) = +inf.  For t = 0 .. n-1:
//   e = emit[w_i, s, sym[t]]
//   a = V(t-1,i,s) + stay[w_i,s]
//   b = s > 0   ?  V(t-1,i,s-1) + adv[w_i,s-1]
//     : i > 0   ?  V(t-1,i-1,S_{i-1}-1) + enter[w_i]
//     : t == 0  ?  0.0 + enter[w_0]
//     :            +inf
//   advance iff b < a (strictly; ties stay)
//   V(t,i,s) = e + (advance ? b : a)
//   score = V(n-1, L-1, S_{L-1}-1)
// dsp_dhmm_decode's cell with the word loop replaced by the transcript's chain; the decoder's free exit is
// kept: adv[c, S-1] stays unread.
// Path.  seg int32 [N, Wmax, Smax]: the first frame of every state of every position, an absolute frame of the
// utterance, walked back from (n-1, L-1, last state) along the advance decisions; -1 for s >= S_i and for
// i >= L.  seg[u, i, 0] is word i's first frame.
// Forced results.  score +inf and the whole seg row -1 when n < 1 or n > T; when L < 1 or L > Wmax; when some
// trans[u, i], i < L, lies outside [0, C) or names a model whose n_states is outside 1 .. Smax; when some
// sym[t], t < n, lies outside [0, K) (such a symbol never indexes a table); and when the recurrence leaves
// +inf (n < sum S_i, a +inf enter, ...).  Either output may be NULL; without seg no direction bit is stored
// and nothing is walked.
// Re-estimation from a GIVEN seg [N, Wmax, Smax]: an utterance is valid when its length and transcript are
// valid as above, every sym[t], t < n, lies in [0, K), and its seg row is well formed: seg[0][0] = 0, strictly
// increasing over the sum S_i concatenated states, the last one < n, and -1 exactly where the definition says.
// Any other utterance is skipped whole (valid[u] = 0).
//   cnt_emit[c,s,k] = frames of valid utterances in state s of an instance of word c that carry symbol k
//   cnt[c,s] likewise over all k;  n_valid[c] = instances of word c in valid utterances;  valid int32 [N]
// Rows s >= S are zeros, as is a model without an instance.  The counts are integers, so the order the device
// adds them in is free.  No floating-point total is formed on the device.
//
// Kernels:
//   dhmm_decode_pack  (hmm_internal.h) the decoder's pack: tab [K][NS][64], tr [NS][64] pairs, j0 [64], by model.
//   dhmm_force<NS, DIR>  one wave per workgroup, one utterance per wave, persistent over the utterances.  A LANE
//              is a transcript position: lane i reads column w_i of the table -- all lanes stay within the
//              512-byte line of (sym[t], slot), lanes with equal words read the same address -- and keeps the
//              NS slots of its word in registers, END-aligned, swept in descending order in place.  Its
//              transitions are read once per utterance: registers for NS <= 16, LDS [slot][lane] for NS = 32.
//              The only coupling between lanes is the entry of position i: lane i-1's exit (slot NS - 1) of
//              the previous frame, taken before the sweep by one DPP lane shift (wave_shr:1); lane 0 keeps
//              (t == 0 ? 0.0 : +inf).  No cross-lane minimum, no barrier.  Emissions one frame ahead and the
//              symbols 64 frames a chunk through the vector path, as in dhmm_decode.  The cell's value is
//              selected by the compare that sets the direction bit (never v_min_f64: -0.0 and +0.0).  DIR: each
//              frame writes one 32-bit word per lane (bit j: slot j advanced) to the wave's [T][64] block of
//              the workspace; the walk back reads a row for all lanes at once, four rows ahead, and follows
//              (lane, slot) by readlane: at most n steps, t strictly decreasing; at the lane's first slot an
//              advance moves to lane - 1, slot NS - 1.
//   force_valid / force_count  the re-estimation: a thread per utterance (the checks, valid, n_valid), a
//              thread per (utterance, position, state) (its run of frames, vector atomic adds on the int32
//              counts); csr_zero zeroes the counts first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "csr_pairs.h"
#include "dsp_audiorec.h"
#include "dtw_internal.h"
#include "hmm_internal.h"

namespace dsp {

static constexpr int DHMM_FORCE_WAVES = 8192;  // persistent waves per launch at most, as dhmm_decode's

static bool force_in_plan(int64_t C, int64_t N, int T, int Wmax, int Smax, int K)
{
    return C >= 1 && C <= DSP_DHMM_DECODE_MAX_MODELS && N >= 0 && N < 0x7fffffff && Smax >= 1 && Smax <= DHMM_SMAX &&
           K >= 1 && K <= DHMM_KMAX && T >= 1 && T <= DTW_TMAX && Wmax >= 1 && Wmax <= DSP_DHMM_FORCE_MAX_WORDS;
}
// the persistent waves of a call: each owns hmm_dir_bytes(T) of direction words
static int force_waves(int64_t N, int T)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(N, DHMM_FORCE_WAVES), (int64_t)(CSR_WAVE_CAP / hmm_dir_bytes(T))));
}
// workspace: [the pack's three parts][direction words of the waves]
static size_t force_bytes(int64_t N, int T, int Smax, int K)
{
    return decode_plan(Smax, K).total() + up256((size_t)force_waves(N, T) * hmm_dir_bytes(T));
}

// lane i takes lane i-1's value; lane 0 has no source and keeps first
__device__ __forceinline__ double force_shift(double x, double first)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(first), __double2loint(x), 0x138, 0xf, 0xf, false);  // wave_shr:1
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(first), __double2hiint(x), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double force_readlane(double x, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}

// slots whose emissions are asked for one frame ahead (dhmm_decode's decode_ahead)
constexpr int force_ahead(int NS) { return NS == 32 ? 16 : NS; }

#pragma clang fp contract(off)
// One frame of the NS slots of every lane's word: v holds frame t-1 and is replaced by frame t.  eh, el: the
// frame's emissions, upper and lower slots; trr / ltr: (stay, cost of coming in) per slot in registers or, for
// NS = 32, in LDS at this lane; j0: the lane's entry slot (NS: never entered); xin: the entry value, the
// position before's exit of frame t-1.  Returns the direction word: bit j = slot j advanced.
template <int NS, bool DIR>
__device__ __forceinline__ uint32_t force_frame(double (&v)[NS], const double (&eh)[force_ahead(NS)],
                                                const double (&el)[NS - force_ahead(NS) + 1],
                                                const double2 (&trr)[NS == 32 ? 1 : NS], const double2 *ltr, int j0, double xin)
{
    constexpr int LO = NS - force_ahead(NS);
    uint32_t md = 0;
    if constexpr (NS == 32) asm volatile("" : "+v"(j0));  // a compare per cell, not 32 masks kept in scalar registers
#pragma unroll
    for (int j = NS - 1; j >= 0; j--) {
        double2 sa;
        if constexpr (NS == 32)
            sa = ltr[j * 64];
        else
            sa = trr[j];
        const double pv = j == j0 ? xin : (j > 0 ? v[j > 0 ? j - 1 : 0] : (double)INFINITY);
        const double a = v[j] + sa.x;
        const double b = pv + sa.y;
        const bool advance = b < a;
        v[j] = (j >= LO ? eh[j >= LO ? j - LO : 0] : el[j < LO ? j : 0]) + (advance ? b : a);
        if (DIR) md |= advance ? 1u << j : 0u;
    }
    return md;
}
#pragma clang fp contract(on)

// CNT slots from slot J0 on of symbol k at this lane's column, the highest first; k is clamped into the table
template <int NS, int J0, int CNT, int LEN>
__device__ __forceinline__ void force_load(double (&e)[LEN], const double *__restrict__ tabl, int k, int K)
{
    const double *__restrict__ row = tabl + (size_t)min((unsigned)k, (unsigned)(K - 1)) * (NS * 64);
#pragma unroll
    for (int j = CNT - 1; j >= 0; j--) e[j] = row[(J0 + j) * 64];
}

template <int NS, bool DIR>
__global__ __launch_bounds__(64) void dhmm_force(const double *__restrict__ tab, const double2 *__restrict__ tr,
                                                 const int32_t *__restrict__ j0s, int C, int Smax, int K,
                                                 const int32_t *__restrict__ sym, const int32_t *__restrict__ len, int N, int T,
                                                 const int32_t *__restrict__ trans, const int32_t *__restrict__ n_trans,
                                                 int Wmax, double *__restrict__ score, int32_t *__restrict__ seg,
                                                 uint32_t *__restrict__ dir_ws)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char force_lds[];
    const int lane = (int)threadIdx.x;
    double2 *ltr = (double2 *)force_lds + lane;
    uint32_t *dir = dir_ws + (size_t)blockIdx.x * (size_t)T * 64 + lane;
    for (int u = (int)blockIdx.x; u < N; u += (int)gridDim.x) {
        const int nraw = len[u], Lraw = n_trans[u];
        const int L = Lraw >= 1 && Lraw <= Wmax ? Lraw : 0;
        // the lane's word: an index outside the set, or a model that is never entered, spoils the transcript
        const int w = trans[(int64_t)u * Wmax + min(lane, Wmax - 1)];
        const int wc = (unsigned)w < (unsigned)C ? w : 0;
        const int jw = j0s[wc];
        const bool mine = lane < L;
        const bool wok = (unsigned)w < (unsigned)C && jw < NS;
        const bool tok = L > 0 && __ballot(mine && !wok) == 0;
        const int n = tok && nraw >= 1 && nraw <= T ? nraw : 0;
        const int j0 = mine && tok ? jw : NS;  // a lane behind the transcript is never entered: its cells stay +inf
        const int32_t *__restrict__ srow = sym + (int64_t)u * T;
        const double *__restrict__ tabl = tab + wc;
        constexpr int PRE = force_ahead(NS), LO = NS - PRE;
        double v[NS], ea[PRE], eb[PRE], el[LO + 1];
        double2 trr[NS == 32 ? 1 : NS];
        if (n > 0) {
            // the word's transitions, once per utterance; a lane reads back only what it wrote itself
#pragma unroll
            for (int j = 0; j < NS; j++) {
                if constexpr (NS == 32)
                    ltr[j * 64] = tr[j * 64 + wc];
                else
                    trr[j] = tr[j * 64 + wc];
            }
        }
#pragma unroll
        for (int j = 0; j < NS; j++) v[j] = INFINITY;
        // 64 symbols a chunk, a lane per frame; the index stays inside the row
        int cur = srow[min(lane, T - 1)];
        bool bad = lane < n && (unsigned)cur >= (unsigned)K;
        int k = __builtin_amdgcn_readlane(cur, 0);
        if (n > 0) force_load<NS, LO, PRE>(ea, tabl, k, K);
        double first = 0.0;  // lane 0's entry: 0.0 at frame 0, +inf after it
        for (int t0 = 0; t0 < n; t0 += 64) {
            const int nxt = srow[min(t0 + 64 + lane, T - 1)];
            bad = bad || (t0 + 64 + lane < n && (unsigned)nxt >= (unsigned)K);
            const int cnt = min(64, n - t0);
            // two frames a turn: the emissions of frame i + 1 are asked for before the cells of frame i
            for (int i = 0; i < cnt; i += 2) {
                force_load<NS, 0, LO>(el, tabl, k, K);
                k = __builtin_amdgcn_readlane(cur, i + 1);
                force_load<NS, LO, PRE>(eb, tabl, k, K);
                uint32_t md = force_frame<NS, DIR>(v, ea, el, trr, ltr, j0, force_shift(v[NS - 1], first));
                if (DIR) dir[(size_t)(t0 + i) * 64] = md;
                first = INFINITY;
                if (i + 1 >= cnt) break;
                force_load<NS, 0, LO>(el, tabl, k, K);
                k = i + 2 < 64 ? __builtin_amdgcn_readlane(cur, (i + 2) & 63) : __builtin_amdgcn_readlane(nxt, 0);
                force_load<NS, LO, PRE>(ea, tabl, k, K);
                md = force_frame<NS, DIR>(v, eb, el, trr, ltr, j0, force_shift(v[NS - 1], first));
                if (DIR) dir[(size_t)(t0 + i + 1) * 64] = md;
            }
            cur = nxt;
        }
        const double x = force_readlane(v[NS - 1], max(L - 1, 0));
        const bool ok = n > 0 && __ballot(bad) == 0 && x < (double)INFINITY;
        if (lane == 0 && score) score[u] = ok ? x : (double)INFINITY;
        if (!DIR) continue;
        // -1 wherever the walk writes nothing: behind the transcript, behind each word's states, a forced row
        int32_t *__restrict__ srowo = seg + (int64_t)u * Wmax * Smax;
        for (int e0 = 0; e0 < Wmax * Smax; e0 += 64) {  // every lane takes every turn: the permute reads all of them
            const int e = e0 + lane, i = min(e / Smax, Wmax - 1), s = e - i * Smax;
            const int Si = NS - __builtin_amdgcn_ds_bpermute(i << 2, j0);  // 0 behind the transcript
            if (e < Wmax * Smax && (!ok || s >= Si)) srowo[e] = -1;
        }
        if (!ok) continue;
        // the walk back from (n-1, lane L-1, slot NS-1): wave-uniform; row r of the words for all lanes at once,
        // four rows asked for before the first is used
        int p = L - 1, j = NS - 1, jp = __builtin_amdgcn_readlane(j0, p);
        for (int r0 = n - 1; r0 >= 0 && p >= 0; r0 -= 4) {
            uint32_t word[4];
#pragma unroll
            for (int q = 0; q < 4; q++) word[q] = dir[(size_t)max(r0 - q, 0) * 64];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int r = r0 - q;
                if (r < 0 || p < 0) break;
                const uint32_t wd = (uint32_t)__builtin_amdgcn_readlane((int)word[q], p);
                if (!((wd >> j) & 1)) continue;
                if (lane == 0) srowo[p * Smax + (j - jp)] = r;
                if (j == jp) {
                    p--;
                    j = NS - 1;
                    jp = __builtin_amdgcn_readlane(j0, max(p, 0));
                } else {
                    j--;
                }
            }
        }
    }
}

// ---- re-estimation ----
// A thread per utterance: valid[u], and for a valid one n_valid of each of its words
__global__ __launch_bounds__(256) void force_valid(const int32_t *__restrict__ n_states, int C, int Smax, int K,
                                                   const int32_t *__restrict__ sym, const int32_t *__restrict__ len, int64_t N,
                                                   int T, const int32_t *__restrict__ trans,
                                                   const int32_t *__restrict__ n_trans, int Wmax,
                                                   const int32_t *__restrict__ seg, int32_t *__restrict__ n_valid,
                                                   int32_t *__restrict__ valid)
{
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < N; u += (int64_t)gridDim.x * 256) {
        const int n = len[u], L = n_trans[u];
        const int32_t *__restrict__ tw = trans + u * Wmax;
        const int32_t *__restrict__ ps = seg + u * Wmax * Smax;
        bool ok = n >= 1 && n <= T && L >= 1 && L <= Wmax;
        int prev = -1;  // the concatenated states' first frames: 0, then strictly increasing, all < n
        for (int i = 0; ok && i < Wmax; i++) {
            int S = 0;
            if (i < L) {
                const int w = tw[i];
                ok = w >= 0 && w < C;
                S = ok ? n_states[w] : 0;
                ok = ok && S >= 1 && S <= Smax;
            }
            for (int s = 0; ok && s < Smax; s++) {
                const int b = ps[i * Smax + s];
                if (s < S) {
                    ok = prev < 0 ? b == 0 : (b > prev && b < n);
                    prev = b;
                } else {
                    ok = b == -1;
                }
            }
        }
        if (ok) {
            const int32_t *__restrict__ sr = sym + u * T;
            unsigned worst = 0;
            for (int t = 0; t < n; t++) worst = max(worst, (unsigned)sr[t]);
            ok = worst < (unsigned)K;
        }
        valid[u] = ok ? 1 : 0;
        if (ok)
            for (int i = 0; i < L; i++) atomicAdd(&n_valid[tw[i]], 1);
    }
}

// A thread per (utterance, position, state): its run of frames, one atomic add per frame on cnt_emit and one
// per run on cnt
__global__ __launch_bounds__(256) void force_count(const int32_t *__restrict__ n_states, int Smax, int K,
                                                   const int32_t *__restrict__ sym, const int32_t *__restrict__ len, int64_t N,
                                                   int T, const int32_t *__restrict__ trans,
                                                   const int32_t *__restrict__ n_trans, int Wmax,
                                                   const int32_t *__restrict__ seg, const int32_t *__restrict__ valid,
                                                   int32_t *__restrict__ cnt_emit, int32_t *__restrict__ cnt)
{
    const int64_t per = (int64_t)Wmax * Smax, total = N * per;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t u = e / per;
        const int r = (int)(e - u * per), i = r / Smax, s = r - i * Smax;
        if (!valid[u]) continue;
        const int L = n_trans[u];
        if (i >= L) continue;
        const int w = trans[u * Wmax + i], S = n_states[w];
        if (s >= S) continue;
        const int32_t *__restrict__ ps = seg + u * per;
        const int b = ps[r];
        const int end = s + 1 < S ? ps[r + 1] : (i + 1 < L ? ps[(i + 1) * Smax] : len[u]);
        const int64_t cs = (int64_t)w * Smax + s;
        const int32_t *__restrict__ sr = sym + u * T;
        for (int t = b; t < end; t++) atomicAdd(&cnt_emit[cs * K + sr[t]], 1);
        atomicAdd(&cnt[cs], end - b);
    }
}

}  // namespace dsp

extern "C" size_t dsp_dhmm_force_workspace_bytes(int64_t C, int64_t N, int T, int Wmax, int Smax, int K)
{
    if (!dsp::force_in_plan(C, N, T, Wmax, Smax, K)) return 0;
    return dsp::force_bytes(N, T, Smax, K);
}

extern "C" int dsp_dhmm_force_align(const double *emit, const double *stay, const double *adv, const int32_t *n_states,
                                    const double *enter, int64_t C, int Smax, int K, const int32_t *sym, const int32_t *len,
                                    int64_t N, int T, const int32_t *trans, const int32_t *n_trans, int Wmax, double *score,
                                    int32_t *seg, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!dsp::force_in_plan(C, N, T, Wmax, Smax, K)) return DSP_ERR_ARGS;
    if (N == 0 || (!score && !seg)) return DSP_OK;
    if (!emit || !stay || !adv || !n_states || !sym || !len || !trans || !n_trans) return DSP_ERR_ARGS;
    if (!workspace || workspace_bytes < dsp::force_bytes(N, T, Smax, K)) return DSP_ERR_WORKSPACE;
    const dsp::DecodePlan pl = dsp::decode_plan(Smax, K);
    hipStream_t s = (hipStream_t)stream;
    const double *tab = (const double *)workspace;
    const double2 *tr = (const double2 *)((char *)workspace + pl.tab);
    const int32_t *j0 = (const int32_t *)((char *)workspace + pl.tab + pl.tr);
    uint32_t *dir = (uint32_t *)((char *)workspace + pl.total());
    dsp::dhmm_decode_pack_launch(s, pl, workspace, emit, stay, adv, n_states, enter, (int)C, Smax, K);
    const int G = dsp::force_waves(N, T);
    const size_t lds = pl.NS == 32 ? (size_t)32 * 64 * 16 : 0;
    dsp::dhmm_with_slots(pl.NS, [&](auto ns) {
        constexpr int SLOTS = decltype(ns)::value;
        if (seg)
            hipLaunchKernelGGL((dsp::dhmm_force<SLOTS, true>), dim3((unsigned)G), dim3(64), lds, s, tab, tr, j0, (int)C, Smax, K, sym,
                               len, (int)N, T, trans, n_trans, Wmax, score, seg, dir);
        else
            hipLaunchKernelGGL((dsp::dhmm_force<SLOTS, false>), dim3((unsigned)G), dim3(64), lds, s, tab, tr, j0, (int)C, Smax, K,
                               sym, len, (int)N, T, trans, n_trans, Wmax, score, seg, dir);
    });
    return dsp::dtw_launch_status();
}

extern "C" int dsp_dhmm_force_accumulate(const int32_t *n_states, int64_t C, int Smax, int K, const int32_t *sym,
                                         const int32_t *len, int64_t N, int T, const int32_t *trans, const int32_t *n_trans,
                                         int Wmax, const int32_t *seg, int32_t *cnt_emit, int32_t *cnt, int32_t *n_valid,
                                         int32_t *valid, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!dsp::force_in_plan(C, N, T, Wmax, Smax, K)) return DSP_ERR_ARGS;
    if (!n_states || !cnt_emit || !cnt || !n_valid || (N > 0 && (!sym || !len || !trans || !n_trans || !seg || !valid)))
        return DSP_ERR_ARGS;
    if (!workspace || workspace_bytes < dsp::force_bytes(N, T, Smax, K)) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(256);
    // cnt_emit, then cnt and n_valid: the caller's three arrays need not be adjacent, so two launches
    hipLaunchKernelGGL((dsp::csr_zero<int32_t, int32_t>), dsp::csr_grid(C * Smax * (int64_t)(K + 1)), block, 0, s, cnt_emit,
                       C * Smax * (int64_t)K, cnt, C * (int64_t)Smax);
    hipLaunchKernelGGL((dsp::csr_zero<int32_t, int32_t>), dsp::csr_grid(C), block, 0, s, n_valid, C, n_valid, (int64_t)0);
    if (N > 0) {
        hipLaunchKernelGGL(dsp::force_valid, dsp::csr_grid(N), block, 0, s, n_states, (int)C, Smax, K, sym, len, N, T, trans,
                           n_trans, Wmax, seg, n_valid, valid);
        hipLaunchKernelGGL(dsp::force_count, dsp::csr_grid(N * Wmax * Smax), block, 0, s, n_states, Smax, K, sym, len, N, T,
                           trans, n_trans, Wmax, seg, valid, cnt_emit, cnt);
    }
    return dsp::dtw_launch_status();
}
