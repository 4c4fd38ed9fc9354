// dhmm_grammar.hip -- connected-word decoding under a word-pair grammar: the one-pass Viterbi of dhmm_decode.hip
// with the cost of a word change depending on the word before, on gfx950 (include/dsp_audiorec.h:
// dsp_dhmm_decode_grammar).  An extension like §4.8-§4.18: nothing here restates a reference
// file.  Every value is defined bit for bit: the device sees only fp64 add and compare.
//
// Inputs.  The model set, sym, len, N, T and max_words of dsp_dhmm_decode with the same value rules and bounds:
// 1 <= C <= 64, Smax <= 32, K <= 256, T <= 1024.  enter float64 [C]: the cost of STARTING THE UTTERANCE with word
// c, NULL means all 0.0.  pair float64 [C, C], row-major: pair[p, c] is the cost of word c following word p;
// required; it carries everything a word change costs, any word penalty included.  leave float64 [C]: the cost
// of ending the utterance on word c, NULL means all 0.0.  All three finite or +inf, never NaN, never -inf; +inf
// forbids.  A model with n_states outside 1 .. Smax is neither a predecessor nor a successor and is never read;
// its cost rows and columns hold anything.
// Recurrence.  The cells are dsp_dhmm_decode's: the value (advance ? b : a) is selected by the same strict
// compare that moves start, ties stay.  Only the entry term of state 0 changes:
//   G(-1, c) = 0.0 + enter[c];  P(-1, c) = -1
//   b at s = 0 of frame t:  G(t-1, c)                       (was X(t-1) + enter[c])
//   E(t, p) = V(t, p, S_p - 1);  Bx(t, p) = start(t, p, S_p - 1)
//   G(t, c) = min over valid p ascending of E(t, p) + pair[p, c], a later p replacing only if strictly smaller
//   P(t, c) = that p (-1 when all are +inf)
//   score   = min over valid c ascending of E(n-1, c) + leave[c], same tie rule;  w = that c
// (The kernel forms b as G(t-1, c) + 0.0 through the packed entry cost.  That has G's bits: x + 0.0 differs from x
// only for x = -0.0, a sum is -0.0 only when both terms are, and G(-1, c) = 0.0 + enter[c] never is, so by
// induction over the frames no V and no G is -0.0.)
// Walk back.  Start at t = n-1 with word w; it starts at b = Bx(t, w); if b = 0 stop; otherwise the word before
// it is P(b-1, w), ending at frame b-1; repeat from there.
// Outputs.  score float64 [N], n_words int32 [N] (the true number), words, start int32 [N, max_words] in time
// order, the first max_words of them, -1 behind them.  The forced rows are dsp_dhmm_decode's: +inf, 0 and -1 rows
// for a bad length, a symbol outside [0, K), or no finite score.  Any output may be NULL.  There is no cum.
//
// Kernels:
//   dhmm_decode_pack  (hmm_internal.h) the decoder's pack with enter NULL: the entry slot's cost of coming in is 0.0.
//   dhmm_grammar<NS>  dhmm_decode's mapping -- one utterance per wave, persistent, a lane per word model -- but 4 (8 slots)
//              or 2 (16, 32 slots) waves to a workgroup, which share the LDS and otherwise never meet; lane c keeps
//              (V, start) of its NS slots in registers; the cell sweep is dhmm_cells.h's decode_cells with the lane's
//              own G as the entry value.  pair sits in LDS as [p][lane] doubles, staged once per workgroup: rows of 512
//              bytes, consecutive lanes at consecutive addresses; the columns of lanes without a valid model and the
//              rows of such predecessors hold +inf, as do the rows up to the next multiple of 8.  After a frame's
//              sweep the (min, +) step runs over p = 0 .. up8(C)-1 in batches of eight LDS reads: predecessor p's
//              exit by a readlane pair (a scalar operand), one add, one strict compare, the selects of value and
//              index.  Every frame stores one 32-bit word per lane, (P(t, c) + 1) << 16 | (Bx(t, c) + 1), to the
//              wave's [T][64] block of the workspace (hmm_dir_bytes(T), as dhmm_force's direction words).  The
//              walk back is wave-uniform, at most n steps with t strictly decreasing: every lane loads its own
//              word of a row and the wanted one is taken by readlane, so no lane reads what another lane wrote.
//              The words are counted first, then those that have a place are written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "csr_pairs.h"
#include "dhmm_cells.h"
#include "dsp_audiorec.h"
#include "dtw_internal.h"
#include "hmm_internal.h"

namespace dsp {

static constexpr int DHMM_GRAMMAR_WAVES = 8192;  // persistent waves per launch at most, as dhmm_decode's

static bool grammar_in_plan(int64_t C, int64_t N, int T, int Smax, int K)
{
    return C >= 1 && C <= DSP_DHMM_DECODE_MAX_MODELS && N >= 0 && N < 0x7fffffff && Smax >= 1 && Smax <= DHMM_SMAX &&
           K >= 1 && K <= DHMM_KMAX && T >= 1 && T <= DTW_TMAX;
}
// waves of a workgroup: they share the LDS copy of pair (and of the transitions), so that the LDS does not set
// the residency below what the registers allow -- 32 KiB of pair a wave would: 5 of 12 waves per CU at 8 slots
// (DESIGN.md §4.19's A / B, profiles/dhmm_grammar_ab.txt).  -DGRAMMAR_WPB=1, 2 or 4 builds that A / B's forms: the
// same number for every slot count.
#ifdef GRAMMAR_WPB
static_assert(GRAMMAR_WPB == 1 || GRAMMAR_WPB == 2 || GRAMMAR_WPB == 4, "GRAMMAR_WPB is 1, 2 or 4");
constexpr int grammar_wpb(int) { return GRAMMAR_WPB; }
#else
constexpr int grammar_wpb(int NS) { return NS == 8 ? 4 : 2; }
#endif
static constexpr int GRAMMAR_WPB_MAX = 4;
// the persistent waves of a call, whole workgroups of them: each owns hmm_dir_bytes(T) of trace words
static int grammar_waves(int64_t N, int T)
{
    const int64_t w = std::min<int64_t>(std::min<int64_t>(N, DHMM_GRAMMAR_WAVES), (int64_t)(CSR_WAVE_CAP / hmm_dir_bytes(T)));
    return (int)(std::max<int64_t>(1, (w + GRAMMAR_WPB_MAX - 1) / GRAMMAR_WPB_MAX) * GRAMMAR_WPB_MAX);
}
// workspace: [the pack's three parts][trace words of the waves]
static size_t grammar_bytes(int64_t N, int T, int Smax, int K)
{
    return decode_plan(Smax, K).total() + up256((size_t)grammar_waves(N, T) * hmm_dir_bytes(T));
}
// rows of pair in LDS: C up to a multiple of 8
static int grammar_rows(int C) { return (C + 7) & ~7; }
// dynamic LDS: the rows of pair, then at 32 slots the transitions
static size_t grammar_lds_bytes(int C, int NS) { return (size_t)grammar_rows(C) * 512 + (NS == 32 ? (size_t)NS * 64 * 16 : 0); }

// The (min, +) step of a frame: G(t, c) and P(t, c) for this lane's c from every lane's exit ev.  lp: the LDS rows
// of pair at this lane, rows (a multiple of 8) of them; rows behind C and lanes behind C hold +inf.
__device__ __forceinline__ void grammar_step(double ev, const double *lp, int rows, double &g, int &pw)
{
#pragma clang fp contract(off)
    g = INFINITY;
    pw = -1;
    for (int p0 = 0; p0 < rows; p0 += 8) {
        double c[8];
#pragma unroll
        for (int q = 0; q < 8; q++) c[q] = lp[(p0 + q) * 64];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const double cand = decode_readlane(ev, p0 + q) + c[q];
            const bool lt = cand < g;
            g = lt ? cand : g;
            pw = lt ? p0 + q : pw;
        }
    }
}

// the word of lane l of a row of trace words, wave-uniform
__device__ __forceinline__ uint32_t grammar_word(uint32_t row, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)row, l); }

template <int NS>
__global__ __launch_bounds__(64 * grammar_wpb(NS)) void dhmm_grammar(const double *__restrict__ tab, const double2 *__restrict__ tr,
                                                   const int32_t *__restrict__ j0s, int C, int K,
                                                   const double *__restrict__ enter, const double *__restrict__ pair,
                                                   const double *__restrict__ leave, const int32_t *__restrict__ sym,
                                                   const int32_t *__restrict__ len, int N, int T, int max_words,
                                                   double *__restrict__ score, int32_t *__restrict__ n_words,
                                                   int32_t *__restrict__ words, int32_t *__restrict__ start,
                                                   uint32_t *__restrict__ trace_ws)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char grammar_lds[];
    constexpr int W = grammar_wpb(NS);
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int wid = (int)blockIdx.x * W + wave, nwaves = (int)gridDim.x * W;
    const int rows = (C + 7) & ~7;
    double *lp = (double *)grammar_lds + lane;
    double2 *ltr = (double2 *)(grammar_lds + (size_t)rows * 512) + lane;
    uint32_t *trace = trace_ws + (size_t)wid * (size_t)T * 64 + lane;
    const double *__restrict__ tabl = tab + lane;
    const int j0 = j0s[lane];
    const bool mine = j0 < NS;  // the lane has a valid model (the pack gives NS to an invalid one and to lanes >= C)
    // enter and leave of the lane's model, loaded only where it is valid (then lane < C)
    double ge = INFINITY, lv = INFINITY;
    if (mine) {
        ge = enter ? enter[lane] : 0.0;
        lv = leave ? leave[lane] : 0.0;
    }
    const double g0 = 0.0 + ge;
    double2 trr[NS == 32 ? 1 : NS];
    // the transitions and pair, once per workgroup: its waves write the LDS rows in turn and meet at one barrier
#pragma unroll
    for (int j = 0; j < NS; j++) {
        if constexpr (NS == 32) {
            if (j % W == wave) ltr[j * 64] = tr[j * 64 + lane];
        } else {
            trr[j] = tr[j * 64 + lane];
        }
    }
    for (int p = wave; p < rows; p += W) {
        const bool pok = p < C && __builtin_amdgcn_readlane(j0, p) < NS;  // wave-uniform: p has a valid model
        double cost = INFINITY;
        if (pok && mine) cost = pair[(size_t)p * C + lane];  // no row and no column of an invalid model is loaded
        lp[p * 64] = cost;
    }
    __syncthreads();  // the only barrier: from here on the LDS is read only and the waves go their own ways
    for (int u = wid; u < N; u += nwaves) {
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
        double g = g0;
        int pw = -1;
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
                decode_cells<NS>(v, st, ea, el, trr, ltr, j0, g, t0 + i);
                grammar_step(v[NS - 1], lp, rows, g, pw);
                trace[(size_t)(t0 + i) * 64] = (uint32_t)(pw + 1) << 16 | (uint32_t)(st[NS - 1] + 1);
                if (i + 1 >= cnt) break;
                decode_load<NS, 0, LO>(el, tabl, k, K);
                k = i + 2 < 64 ? __builtin_amdgcn_readlane(cur, (i + 2) & 63) : __builtin_amdgcn_readlane(nxt, 0);
                decode_load<NS, LO, PRE>(ea, tabl, k, K);
                decode_cells<NS>(v, st, eb, el, trr, ltr, j0, g, t0 + i + 1);
                grammar_step(v[NS - 1], lp, rows, g, pw);
                trace[(size_t)(t0 + i + 1) * 64] = (uint32_t)(pw + 1) << 16 | (uint32_t)(st[NS - 1] + 1);
            }
            cur = nxt;
        }
        // the end: the smallest E(n-1, c) + leave[c], the smallest c among equals
        double x = INFINITY;
        int w = 0;
        {
#pragma clang fp contract(off)
            const double fin = v[NS - 1] + lv;
            const double m = decode_wave_min(fin);
            const unsigned long long eq = __ballot(fin == m);
            w = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(eq | (1ull << 63)));
            x = m < (double)INFINITY ? decode_readlane(fin, w) : (double)INFINITY;
        }
        const bool ok = n > 0 && __ballot(bad) == 0 && x < (double)INFINITY;
        // the walk back, the same for every lane: first the number of words ...
        int nw = 0;
        if (ok) {
            int t = n - 1, wc = w;
            for (int step = 0; step < n; step++) {
                const uint32_t row = trace[(size_t)t * 64];
                if (step > 0) {
                    const int p = (int)(grammar_word(row, wc) >> 16) - 1;
                    if (p < 0) break;  // not reached with the sweep's own words
                    wc = min(p, 63);
                }
                const int b = (int)(grammar_word(row, wc) & 0xffffu) - 1;
                nw++;
                if (b <= 0) break;
                t = min(b, t) - 1;
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
        }
        // ... then the words, last first, those of them that have a place
        if (ok && (words || start)) {
            int t = n - 1, wc = w;
            for (int i = nw - 1; i >= 0; i--) {
                const uint32_t row = trace[(size_t)t * 64];
                if (i < nw - 1) wc = min(max((int)(grammar_word(row, wc) >> 16) - 1, 0), 63);
                const int b = (int)(grammar_word(row, wc) & 0xffffu) - 1;
                if (lane == 0 && i < max_words) {
                    if (words) words[o + i] = wc;
                    if (start) start[o + i] = b;
                }
                if (b <= 0) break;
                t = min(b, t) - 1;
            }
        }
    }
}

}  // namespace dsp

extern "C" size_t dsp_dhmm_decode_grammar_workspace_bytes(int64_t C, int64_t N, int T, int Smax, int K)
{
    if (!dsp::grammar_in_plan(C, N, T, Smax, K)) return 0;
    return dsp::grammar_bytes(N, T, Smax, K);
}

extern "C" int dsp_dhmm_decode_grammar(const double *emit, const double *stay, const double *adv, const int32_t *n_states,
                                       const double *enter, const double *pair, const double *leave, int64_t C, int Smax,
                                       int K, const int32_t *sym, const int32_t *len, int64_t N, int T, int max_words,
                                       double *score, int32_t *n_words, int32_t *words, int32_t *start, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    if (!dsp::grammar_in_plan(C, N, T, Smax, K) || max_words < 1 || max_words > T) return DSP_ERR_ARGS;
    if (N == 0 || (!score && !n_words && !words && !start)) return DSP_OK;
    if (!emit || !stay || !adv || !n_states || !pair || !sym || !len) return DSP_ERR_ARGS;
    if (!workspace || workspace_bytes < dsp::grammar_bytes(N, T, Smax, K)) return DSP_ERR_WORKSPACE;
    const dsp::DecodePlan pl = dsp::decode_plan(Smax, K);
    hipStream_t s = (hipStream_t)stream;
    const double *tab = (const double *)workspace;
    const double2 *tr = (const double2 *)((char *)workspace + pl.tab);
    const int32_t *j0 = (const int32_t *)((char *)workspace + pl.tab + pl.tr);
    uint32_t *trace = (uint32_t *)((char *)workspace + pl.total());
    // enter NULL: the entry slot's cost of coming in is 0.0, the grammar's costs are in G
    dsp::dhmm_decode_pack_launch(s, pl, workspace, emit, stay, adv, n_states, nullptr, (int)C, Smax, K);
    const int G = dsp::grammar_waves(N, T);
    const size_t lds = dsp::grammar_lds_bytes((int)C, pl.NS);
    dsp::dhmm_with_slots(pl.NS, [&](auto ns) {
        constexpr int SLOTS = decltype(ns)::value, W = dsp::grammar_wpb(SLOTS);
        hipLaunchKernelGGL(dsp::dhmm_grammar<SLOTS>, dim3((unsigned)(G / W)), dim3(64 * W), lds, s, tab, tr, j0, (int)C, K, enter,
                           pair, leave, sym, len, (int)N, T, max_words, score, n_words, words, start, trace);
    });
    return dsp::dtw_launch_status();
}
