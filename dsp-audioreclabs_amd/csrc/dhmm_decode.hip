// dhmm_decode.hip -- connected-word decoding: the one-pass (token-passing) Viterbi over a loop of the
// word models of a discrete-HMM set (dhmm.hip), on gfx950 (include/dsp_audiorec.h: dsp_dhmm_decode;
// DESIGN.md §4.15).  An extension like §4.8-§4.14: nothing here restates a reference file.  Every value
// is defined bit for bit: the device sees only fp64 add and compare.
//
// Inputs.  The model set of dsp_dhmm_score with the same value rules: emit float64 [C, Smax, K], stay,
// adv float64 [C, Smax], n_states int32 [C]; adv[c, S-1] stays unread: leaving a word's last state is
// free.  enter float64 [C] is the cost of starting word c, finite or +inf, never NaN, never -inf; NULL
// means all 0.0.  A model with n_states[c] outside 1 .. Smax counts as enter[c] = +inf: it is never
// entered and never read.  1 <= C <= 64, Smax <= 32, K <= 256; sym int32 [N, T], len int32 [N], T <= 1024.
// Recurrence.  For an utterance of n frames every cell is (V, start), with V(-1, ., .) = +inf and
// X(-1) = 0.0.  For t = 0 .. n-1, model c with S = n_states[c], state s:
//   e = emit[c, s, sym[t]]
//   a = V(t-1,c,s) + stay[c,s]
//   b = s > 0 ?  V(t-1,c,s-1) + adv[c,s-1]  :  X(t-1) + enter[c]
//   advance iff b < a (strictly; ties stay)
//   V(t,c,s)     = e + (advance ? b : a)
//   start(t,c,s) = advance ? (s > 0 ? start(t-1,c,s-1) : t) : start(t-1,c,s)
//   X(t) = min over c ascending of V(t,c,S_c-1), a later c replacing only if strictly smaller
//   W(t) = that c (-1 when every exit is +inf)
//   B(t) = start(t, W(t), S_W-1)
// Result.  score = X(n-1); the words are walked back: t = n-1, the word is W(t) and starts at B(t), then
// t = B(t) - 1, until t < 0.  score float64 [N], n_words int32 [N] (the true number), words, start int32
// [N, max_words], cum float64 [N, max_words] (X at each word's last frame) in time order, the first
// max_words of them; -1 (cum: +inf) behind the words.  score +inf, n_words 0 and -1 / +inf rows when
// n < 1 or n > T, when any sym[t], t < n, lies outside [0, K) (the index is clamped and the result
// forced), and when no word can end at n-1.
//
// Kernels:
//   dhmm_decode_pack  (hmm_internal.h, with the plan of its three parts; dhmm_force.hip launches it too) the
//              set transposed into the workspace for a wave whose LANE is the word model:
//              tab [K][NS][64] doubles, NS = 8, 16 or 32 slots as in dhmm.hip and END-aligned (state s of a
//              model of S states in slot s + NS - S, so every model's exit is slot NS - 1); the slots before
//              a model's first state, a model with an invalid n_states and the lanes c >= C hold +inf, so
//              their cells start at +inf and stay there.  tr [NS][64] pairs (stay, cost of coming in from
//              the slot before): adv[s-1], and at the model's first slot enter[c].  j0 [64]: that first
//              slot, NS where the model is never entered.
//   dhmm_decode<NS>  one wave per workgroup, one utterance per wave, persistent over the utterances.  Lane
//              c keeps V and start of its NS slots in registers and sweeps them in descending order in
//              place.  A frame's emissions are the row of ONE symbol for every lane: NS coalesced loads of
//              512 contiguous bytes, issued one frame ahead into a second register set (the frame loop is
//              unrolled by two, so the sets swap without a move; at 32 slots only the upper 16, see
//              decode_ahead).  The cell sweep, the loads and the minimum are dhmm_cells.h's, which
//              dhmm_grammar.hip uses too.  The predecessor of slot j is slot j-1
//              or, at the lane's own j0, the entry (X(t-1), start t): one per-slot select.  The symbols
//              come 64 frames at a time through the vector path (a lane per frame, the next 64 one chunk
//              ahead) and a frame's symbol by a readlane: no scalar load in the frame loop.  Transitions:
//              registers for NS <= 16; for NS = 32 LDS as [slot][lane] 16-byte pairs, consecutive lanes at
//              consecutive addresses.  The exit: a 64-lane min by DPP moves within each row of 16 lanes
//              and four readlanes, then the ballot of (exit == min), whose lowest set bit is the smallest
//              model index -- the tie rule; X and B are that lane's values by readlane.  (X, W, B) of the
//              frame go to LDS, 16 bytes per frame; after the last frame the wave walks them back, once to
//              count the words and once to write them.  Every loop is bounded by n <= T.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dhmm_cells.h"
#include "dsp_audiorec.h"
#include "dtw_internal.h"
#include "hmm_internal.h"

namespace dsp {

static constexpr int DHMM_DECODE_WAVES = 8192;  // persistent waves per launch at most (32 per CU, all that can be resident)

static bool decode_in_plan(int64_t C, int64_t N, int T, int Smax, int K)
{
    return C >= 1 && C <= DSP_DHMM_DECODE_MAX_MODELS && N >= 0 && N < 0x7fffffff && Smax >= 1 && Smax <= DHMM_SMAX &&
           K >= 1 && K <= DHMM_KMAX && T >= 1 && T <= DTW_TMAX;
}
// dynamic LDS: 16 bytes per frame, then at 32 slots the transitions
static size_t decode_lds_bytes(int T, int NS) { return (size_t)T * 16 + (NS == 32 ? (size_t)NS * 64 * 16 : 0); }

#pragma clang fp contract(off)
// One frame: decode_cells (dhmm_cells.h, its arguments passed on, xprev = X(t-1)), then the exit: (X, W, B) of
// frame t to fr[t] by lane 0, X(t) returned.
template <int NS>
__device__ __forceinline__ double decode_frame(double (&v)[NS], int (&st)[NS], const double (&eh)[decode_ahead(NS)],
                                               const double (&el)[NS - decode_ahead(NS) + 1],
                                               const double2 (&trr)[NS == 32 ? 1 : NS], const double2 *ltr, int j0,
                                               double xprev, int t, int lane, int4 *fr)
{
    decode_cells<NS>(v, st, eh, el, trr, ltr, j0, xprev, t);
    const double ev = v[NS - 1];
    const double m = decode_wave_min(ev);
    const bool any = m < (double)INFINITY;
    const unsigned long long eq = __ballot(ev == m);
    const int w = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(eq | (1ull << 63)));
    const double x = any ? decode_readlane(ev, w) : (double)INFINITY;
    const int b = any ? __builtin_amdgcn_readlane(st[NS - 1], w) : -1;
    if (lane == 0) fr[t] = make_int4(__double2loint(x), __double2hiint(x), any ? w : -1, b);
    return x;
}
#pragma clang fp contract(on)

template <int NS>
__global__ __launch_bounds__(64) void dhmm_decode(const double *__restrict__ tab, const double2 *__restrict__ tr,
                                                  const int32_t *__restrict__ j0s, int K, const int32_t *__restrict__ sym,
                                                  const int32_t *__restrict__ len, int N, int T, int max_words,
                                                  double *__restrict__ score, int32_t *__restrict__ n_words,
                                                  int32_t *__restrict__ words, int32_t *__restrict__ start,
                                                  double *__restrict__ cum)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char decode_lds[];
    const int lane = (int)threadIdx.x;
    int4 *fr = (int4 *)decode_lds;
    double2 *ltr = (double2 *)(decode_lds + (size_t)T * 16) + lane;
    const double *__restrict__ tabl = tab + lane;
    const int j0 = j0s[lane];
    double2 trr[NS == 32 ? 1 : NS];
    // the lane's transitions, once per wave; a lane reads back only what it wrote itself
#pragma unroll
    for (int j = 0; j < NS; j++) {
        if constexpr (NS == 32)
            ltr[j * 64] = tr[j * 64 + lane];
        else
            trr[j] = tr[j * 64 + lane];
    }
    for (int u = (int)blockIdx.x; u < N; u += (int)gridDim.x) {
        const int nraw = len[u];
        const int n = nraw >= 1 && nraw <= T ? nraw : 0;
        const int32_t *__restrict__ srow = sym + (int64_t)u * T;
        constexpr int PRE = decode_ahead(NS), LO = NS - PRE;
        double v[NS], ea[PRE], eb[PRE], el[LO + 1];
        int st[NS];
#pragma unroll
        for (int j = 0; j < NS; j++) {
            v[j] = INFINITY;
            st[j] = -1;
        }
        double x = 0.0;
        // 64 symbols a chunk, a lane per frame; the index stays inside the row
        int cur = srow[min(lane, T - 1)];
        bool bad = lane < n && (unsigned)cur >= (unsigned)K;
        int k = __builtin_amdgcn_readlane(cur, 0);
        decode_load<NS, LO, PRE>(ea, tabl, k, K);
        for (int t0 = 0; t0 < n; t0 += 64) {
            const int nxt = srow[min(t0 + 64 + lane, T - 1)];
            bad = bad || (t0 + 64 + lane < n && (unsigned)nxt >= (unsigned)K);
            const int cnt = min(64, n - t0);
            // two frames a turn: the emissions of frame i + 1 are asked for before the cells of frame i
            for (int i = 0; i < cnt; i += 2) {
                decode_load<NS, 0, LO>(el, tabl, k, K);
                k = __builtin_amdgcn_readlane(cur, i + 1);
                decode_load<NS, LO, PRE>(eb, tabl, k, K);
                x = decode_frame<NS>(v, st, ea, el, trr, ltr, j0, x, t0 + i, lane, fr);
                if (i + 1 >= cnt) break;
                decode_load<NS, 0, LO>(el, tabl, k, K);
                k = i + 2 < 64 ? __builtin_amdgcn_readlane(cur, (i + 2) & 63) : __builtin_amdgcn_readlane(nxt, 0);
                decode_load<NS, LO, PRE>(ea, tabl, k, K);
                x = decode_frame<NS>(v, st, eb, el, trr, ltr, j0, x, t0 + i + 1, lane, fr);
            }
            cur = nxt;
        }
        __syncthreads();  // one wave: lane 0's frame records are visible to every lane
        const bool ok = n > 0 && __ballot(bad) == 0 && x < (double)INFINITY;
        // the walk back, the same for every lane: first the number of words ...
        int nw = 0;
        if (ok) {
            int t = n - 1;
            for (int step = 0; step < n && t >= 0; step++) {
                nw++;
                t = min(fr[t].w, t) - 1;
            }
        }
        if (lane == 0) {
            if (score) score[u] = ok ? x : (double)INFINITY;
            if (n_words) n_words[u] = nw;
        }
        const int64_t o = (int64_t)u * max_words;
        for (int i = lane; i < max_words; i += 64) {
            if (i < nw) continue;
            if (words) words[o + i] = -1;
            if (start) start[o + i] = -1;
            if (cum) cum[o + i] = INFINITY;
        }
        // ... then the words, last first, those of them that have a place
        if (ok && lane == 0) {
            int t = n - 1;
            for (int i = nw - 1; i >= 0 && t >= 0; i--) {
                const int4 r = fr[t];
                if (i < max_words) {
                    if (words) words[o + i] = r.z;
                    if (start) start[o + i] = r.w;
                    if (cum) cum[o + i] = __hiloint2double(r.y, r.x);
                }
                t = min(r.w, t) - 1;
            }
        }
        __syncthreads();  // the records are read before the next utterance's frames replace them
    }
}

}  // namespace dsp

extern "C" size_t dsp_dhmm_decode_workspace_bytes(int64_t C, int64_t N, int T, int Smax, int K)
{
    if (!dsp::decode_in_plan(C, N, T, Smax, K)) return 0;
    return dsp::decode_plan(Smax, K).total();
}

extern "C" int dsp_dhmm_decode(const double *emit, const double *stay, const double *adv, const int32_t *n_states,
                               const double *enter, int64_t C, int Smax, int K, const int32_t *sym, const int32_t *len,
                               int64_t N, int T, int max_words, double *score, int32_t *n_words, int32_t *words,
                               int32_t *start, double *cum, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!dsp::decode_in_plan(C, N, T, Smax, K) || max_words < 1 || max_words > T) return DSP_ERR_ARGS;
    if (N == 0 || (!score && !n_words && !words && !start && !cum)) return DSP_OK;
    if (!emit || !stay || !adv || !n_states || !sym || !len) return DSP_ERR_ARGS;
    const dsp::DecodePlan pl = dsp::decode_plan(Smax, K);
    if (!workspace || workspace_bytes < pl.total()) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double *tab = (double *)workspace;
    double2 *tr = (double2 *)((char *)workspace + pl.tab);
    int32_t *j0 = (int32_t *)((char *)workspace + pl.tab + pl.tr);
    const int NS = pl.NS;
    dsp::dhmm_decode_pack_launch(s, pl, workspace, emit, stay, adv, n_states, enter, (int)C, Smax, K);
    const int G = (int)std::min<int64_t>(N, dsp::DHMM_DECODE_WAVES);
    const size_t lds = dsp::decode_lds_bytes(T, NS);
    dsp::dhmm_with_slots(NS, [&](auto ns) {
        hipLaunchKernelGGL(dsp::dhmm_decode<decltype(ns)::value>, dim3((unsigned)G), dim3(64), lds, s, tab, tr, j0, K, sym, len,
                           (int)N, T, max_words, score, n_words, words, start, cum);
    });
    return dsp::dtw_launch_status();
}
