// dhmm.hip -- left-to-right hidden Markov models with DISCRETE observations (a symbol per frame, the
// output of a shared VQ codebook), in the negative-log domain, on gfx950 (include/dsp_audiorec.h:
// dsp_dhmm_score, dsp_dhmm_align, dsp_dhmm_accumulate).  An extension like §4.8-§4.13:
// nothing here restates a reference file.  Every value is defined bit for bit: the device sees only
// fp64 add and min and integer counts; the logarithms are taken on the host when the model is built.
//
// Symbols.  sym int32 [N, T] padded row-major with len int32 [N], 1 <= T <= 1024: the layout of
// dsp_vq_assign's code for members = 0 .. N-1 of one group.  Entries at t >= len are never read through.
// Alphabet.  K symbols, 1 <= K <= 256, shared by all models of a set.
// Model set.  C models padded to Smax <= 32 states, 1 <= n_states[c] <= Smax: emit float64 [C, Smax, K]
// (= -log b_s(k)), stay, adv float64 [C, Smax], all finite or +inf, never NaN, never -inf; adv[c, S-1]
// and the rows s >= S are never read.
// Recurrence, for a sequence of length n and a model of S states (fp64 add and min only, each rounded):
//   e(t,s)  = emit[c, s, sym[t]]
//   V(0,0)  = e(0,0);  V(0,s>0) = +inf
//   a = V(t-1,s) + stay[s];  b = V(t-1,s-1) + adv[s-1]   (b = +inf at s = 0)
//   V(t,s)  = e(t,s) + min(a, b)
//   score   = V(n-1, S-1)
// The score is +inf when n < S (it comes out of the recurrence), when n < 1 or n > T, when n_states is
// outside 1 .. Smax, for a list entry outside [0, N), and when any sym[t], t < n, lies outside [0, K):
// such a symbol never indexes the table (the index is clamped and the result forced).
// Path.  hmm.hip's (hmm_internal.h's hmm_walk_back): walk back from (n-1, S-1), the predecessor is the advance iff b < a
// strictly; seg int32 [P, Smax], seg[s] the first frame of state s, -1 behind the model's states and
// everywhere for a pair whose score is +inf.
// Re-estimation from a GIVEN seg [P, Smax] and score [P]: a member is valid when its index and length
// are, its seg row is well formed for its model (seg[0] = 0, strictly increasing over the S states,
// seg[S-1] < n) and every sym[t], t < n, lies in [0, K); any other member is skipped whole.
//   cnt_emit[c,s,k] = frames of valid members in state s that carry symbol k;  cnt[c,s] likewise over all k
//   n_valid[c] = valid members;  total[c] = their scores added in list order, the first the value itself
// Rows s >= S are zeros; a model without a valid member or with an invalid n_states has all-zero counts,
// total 0.0 and n_valid 0.  The counts are integers, so the order the device adds them in is free.
//
// Kernels (the record, its staging and the seg rows are hmm_internal.h's):
//   dhmm_dp<NS, DIR>  hmm_dp's shape: one persistent wave per tile of ONE model and 64 sequences, a lane
//              per sequence, the tiles from csr_pairs.h's csr_walk; the NS cells of a lane in registers
//              (NS = 8, 16 or 32 slots, the smallest that holds Smax), the state loop fully unrolled, slots
//              swept in descending order in place; the lane's symbol one row ahead through the vector path.
//              The record is staged into LDS when the tile's model is not the one staged last.  A row is
//              NS / 2 ds_read_b128 of the lane's own symbol's slots (a true gather, two states per read) and
//              NS broadcast ds_read_b128 of (stay, adv[s-1]); no scalar load in the loop, so the waits are
//              counted lgkmcnt.  4 fp64 instructions per cell; DIR as hmm_dp's.
//   csr_label  (csr_pairs.h) the label of a score matrix.
//   dhmm_pairs / dhmm_count / dhmm_totals   the re-estimation: a thread per pair (its model, the seg row
//              and symbol range checks), a thread per (pair, frame) (the frame's state from the seg row,
//              vector atomic adds on the int32 counts), a thread per model (the ordered total and n_valid);
//              csr_zero zeroes the counts first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "csr_pairs.h"
#include "dsp_audiorec.h"
#include "dtw_internal.h"
#include "hmm_internal.h"

namespace dsp {

#pragma clang fp contract(off)
// One row of the NS slots: v holds row t-1 and is replaced by row t; erow: the slots of the lane's own
// symbol in LDS; tr: (stay, adv[s-1]) per slot in LDS, the same address for every lane.  FIRST: row 0,
// slot j0 (state 0) starts the path.  DIR: bit j of word = "the predecessor of slot j is the advance".
template <int NS, bool FIRST, bool DIR>
__device__ __forceinline__ void dhmm_row(double (&v)[NS], const double2 *erow, const double2 *tr, int j0, uint32_t &word)
{
    uint32_t md = 0;
    double2 e2[NS / 2];
    // the row's gather is issued before its cells: NS / 2 reads in flight, consumed in descending order
#pragma unroll
    for (int i = NS / 2 - 1; i >= 0; i--) e2[i] = erow[i];
    // slots in descending order: slot j reads row t-1 of slots j and j-1 only, so it is replaced in place
#pragma unroll
    for (int j = NS - 1; j >= 0; j--) {
        const double e = (j & 1) ? e2[j / 2].y : e2[j / 2].x;
        if (FIRST) {
            v[j] = j == j0 ? e : (double)INFINITY;
        } else {
            const double2 sa = tr[j];
            const double a = v[j] + sa.x;
            const double b = (j > 0 ? v[j - 1] : (double)INFINITY) + sa.y;
            // md = 2 md + (b < a): the compare's bit shifted in through the carry
            if (DIR)
                asm("v_cmp_lt_f64 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(md) : "v"(b), "v"(a) : "vcc");
            v[j] = e + dtw_min(a, b);
        }
    }
    if (DIR) word = md;
}

// V(n-1, S-1) of the lane's symbol row sr (n its length, 0: nothing of the lane is used) under the model
// staged in LDS (tab: its table, tr: its transitions), state 0 in slot j0; nmax > 0 the wave's largest n.
// A symbol outside [0, K) at t < n forces +inf; its index is clamped.  dir: this wave's direction words
// at this lane, [row][lane]; NULL: not stored.
template <int NS, bool DIR>
__device__ __forceinline__ double dhmm_sweep(const unsigned char *tab, const double2 *tr, int j0, int K,
                                             const int32_t *__restrict__ sr, int n, int nmax, uint32_t *dir)
{
    double v[NS];
    uint32_t word = 0;
    auto row_of = [&](int k) { return (const double2 *)(tab + (unsigned)min((unsigned)k, (unsigned)(K - 1)) * dhmm_pitch(NS)); };
    int k = sr[0];
    bool bad = n >= 1 && (unsigned)k >= (unsigned)K;
    dhmm_row<NS, true, DIR>(v, row_of(k), tr, j0, word);
    if (DIR && dir) dir[0] = 0;
    double res = n == 1 ? v[NS - 1] : (double)INFINITY;
    k = sr[min(1, nmax - 1)];
    for (int t = 1; t < nmax; t++) {
        const int kn = sr[min(t + 1, nmax - 1)];  // the next row's symbol, asked for before this row's cells
        bad = bad || (t < n && (unsigned)k >= (unsigned)K);
        dhmm_row<NS, false, DIR>(v, row_of(k), tr, j0, word);
        if (DIR && dir) dir[(size_t)t * 64] = word;
        if (t == n - 1) res = v[NS - 1];
        k = kn;
    }
    return bad ? (double)INFINITY : res;
}
#pragma clang fp contract(on)

// The models c = 0 .. nc-1 of this launch (rec, n_states and group_start already point at the first
// one, model c0 of the set).  group_start == NULL: every model against all N sequences, the result
// of (sequence r, model c) at score[r * C + c0 + c]; else the CSR pairs, outputs indexed by p.
// Dynamic LDS: dhmm_lds_bytes(K, NS).  At 32 slots the LDS lets about two waves per SIMD stay
// resident anyway (K = 64: nine tables per CU), so the scheduler is told to plan for two: with the
// registers that frees it keeps up to 14 transition reads in flight instead of one.
template <int NS, bool DIR>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, NS == 32 ? 2 : 8))) void dhmm_dp(const double *__restrict__ rec, const int32_t *__restrict__ n_states, int c0,
                                              int nc, int64_t C, int Smax, int K, const int32_t *__restrict__ sym,
                                              const int32_t *__restrict__ len, int64_t N, int T,
                                              const int32_t *__restrict__ group_start,
                                              const int32_t *__restrict__ members, int P, double *__restrict__ score,
                                              int32_t *__restrict__ seg, uint32_t *dir_ws)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dhmm_lds[];
    const int lane = (int)threadIdx.x, wv = (int)blockIdx.x;
    const double2 *tr = (const double2 *)(dhmm_lds + dhmm_tr_offset(K, NS));
    uint32_t *dir = DIR && seg ? dir_ws + (size_t)wv * (size_t)T * 64 + lane : nullptr;
    int staged = -1;
    csr_walk((int)gridDim.x, wv, nc, group_start, 0, group_start ? P : (int)N, members, len, N, T,
             [&](int cg, const CsrLane &ln) {
                 const int S = n_states[cg], n = ln.len;
                 const bool sok = S >= 1 && S <= Smax;
                 const int64_t p = ln.p;
                 double res = INFINITY;
                 if (sok && ln.lmax > 0) {
                     if (staged != cg) {
                         dhmm_stage<NS>(dhmm_lds, rec + (size_t)cg * dhmm_record(K, NS), K, lane);
                         staged = cg;
                     }
                     res = dhmm_sweep<NS, DIR>(dhmm_lds, tr, NS - S, K, sym + (int64_t)ln.row * T, n, ln.lmax, dir);
                 }
                 if (!ln.inr) return;
                 if (score) score[group_start ? p : p * C + c0 + cg] = res;
                 if (DIR && seg) hmm_walk_back(dir, n, S, NS, Smax, res < INFINITY, seg + p * Smax);
             });
}

// ---- re-estimation ----
// A thread per pair: pmodel[p] = its model (the group that holds p) when the member is valid, else -1.
__global__ __launch_bounds__(256) void dhmm_pairs(const int32_t *__restrict__ n_states, int64_t C, int Smax, int K,
                                                  const int32_t *__restrict__ sym, const int32_t *__restrict__ len,
                                                  int64_t N, int T, const int32_t *__restrict__ group_start,
                                                  const int32_t *__restrict__ members, int64_t P,
                                                  const int32_t *__restrict__ seg, int32_t *__restrict__ pmodel)
{
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
        const int64_t lo = csr_group_of(group_start, C, p);
        const int S = n_states[lo], mem = members[p];
        const int32_t *__restrict__ ps = seg + p * Smax;
        bool ok = S >= 1 && S <= Smax && mem >= 0 && mem < N && p >= group_start[lo] && p < group_start[lo + 1];
        const int n = ok ? len[mem] : 0;
        ok = ok && n >= 1 && n <= T && hmm_seg_ok(ps, S, n);
        if (ok) {
            const int32_t *__restrict__ sr = sym + (int64_t)mem * T;
            unsigned worst = 0;
            for (int t = 0; t < n; t++) worst = max(worst, (unsigned)sr[t]);
            ok = worst < (unsigned)K;
        }
        pmodel[p] = ok ? (int32_t)lo : -1;
    }
}

// A thread per (pair, frame): the frame's state from the seg row; one atomic add per frame on cnt_emit
// and one per (pair, state) on cnt (the state's first frame adds its length).
__global__ __launch_bounds__(256) void dhmm_count(const int32_t *__restrict__ n_states, int Smax, int K,
                                                  const int32_t *__restrict__ sym, const int32_t *__restrict__ len, int T,
                                                  const int32_t *__restrict__ members, int64_t P,
                                                  const int32_t *__restrict__ seg, const int32_t *__restrict__ pmodel,
                                                  int32_t *__restrict__ cnt_emit, int32_t *__restrict__ cnt)
{
    const int64_t total = P * T;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t p = e / T;
        const int t = (int)(e % T), c = pmodel[p];
        if (c < 0) continue;
        const int mem = members[p], n = len[mem];
        if (t >= n) continue;
        const int S = n_states[c];
        const int32_t *__restrict__ ps = seg + p * Smax;
        int s = 0;
        while (s + 1 < S && ps[s + 1] <= t) s++;
        const int64_t cs = (int64_t)c * Smax + s;
        atomicAdd(&cnt_emit[cs * K + sym[(int64_t)mem * T + t]], 1);
        if (t == ps[s]) atomicAdd(&cnt[cs], (s + 1 < S ? ps[s + 1] : n) - t);
    }
}

#pragma clang fp contract(off)
// A thread per model: n_valid and total, the valid members' scores added in list order
__global__ __launch_bounds__(256) void dhmm_totals(int64_t C, const int32_t *__restrict__ group_start, int64_t P,
                                                   const int32_t *__restrict__ pmodel, const double *__restrict__ score,
                                                   int32_t *__restrict__ n_valid, double *__restrict__ total_out)
{
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < C; c += (int64_t)gridDim.x * 256) {
        const int g0 = clampi(group_start[c], 0, (int)P), g1 = clampi(group_start[c + 1], 0, (int)P);
        int nv = 0;
        double tot = 0.0;
        for (int p0 = g0; p0 < g1; p0 += HMM_BATCH) {
            bool ok[HMM_BATCH];
            double sc[HMM_BATCH];
#pragma unroll
            for (int u = 0; u < HMM_BATCH; u++) {
                const bool in_group = p0 + u < g1;
                ok[u] = in_group && pmodel[p0 + u] == c;
                sc[u] = in_group ? score[p0 + u] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < HMM_BATCH; u++) {
                if (!ok[u]) continue;
                tot = nv == 0 ? sc[u] : tot + sc[u];
                nv++;
            }
        }
        n_valid[c] = nv;
        total_out[c] = tot;
    }
}
#pragma clang fp contract(on)

// ---- host side ----
// workspace: [records of the C models][direction words of G waves][score [N, C], for labels without
// scores][the pairs' models: dsp_dhmm_accumulate]
struct DhmmPlan {
    int NS, G;
    size_t rec, dir, score, pmodel;
    size_t total() const { return rec + dir + score + pmodel; }
};
static DhmmPlan dhmm_plan(int64_t C, int64_t N, int64_t P, int T, int Smax, int K)
{
    DhmmPlan pl;
    pl.NS = dhmm_slots(Smax);
    pl.G = csr_waves(P / 64 + std::min<int64_t>(C, HMM_GCHUNK), hmm_dir_bytes(T));
    pl.rec = up256((size_t)C * dhmm_record(K, pl.NS) * 8);
    pl.dir = up256(pl.G * hmm_dir_bytes(T));
    pl.score = up256((size_t)N * C * 8);
    pl.pmodel = up256((size_t)P * 4);
    return pl;
}

// the records, then the DP over all models in launches of at most HMM_GCHUNK
template <bool DIR>
static int dhmm_run(hipStream_t s, const DhmmPlan &pl, void *ws, const double *emit, const double *stay, const double *adv,
                    const int32_t *n_states, int64_t C, int Smax, int K, const int32_t *sym, const int32_t *len, int64_t N,
                    int T, const int32_t *group_start, const int32_t *members, int64_t P, double *score, int32_t *seg)
{
    double *rec = (double *)ws;
    uint32_t *dir = (uint32_t *)((char *)ws + pl.rec);
    const int NS = pl.NS;
    const size_t R = dhmm_record(K, NS), lds = dhmm_lds_bytes(K, NS);
    hipLaunchKernelGGL(dhmm_pack, csr_grid(C * (int64_t)R), dim3(256), 0, s, emit, stay, adv, n_states, C, Smax, K, NS, rec);
    for (int64_t c0 = 0; c0 < C; c0 += HMM_GCHUNK) {
        const int64_t nc = std::min<int64_t>(HMM_GCHUNK, C - c0);
        const int64_t tiles = group_start ? P / 64 + nc : nc * ((N + 63) / 64);
        const int G = DIR ? std::min(pl.G, csr_waves(tiles, hmm_dir_bytes(T))) : csr_waves(tiles, 0);
        const double *rc = rec + (size_t)c0 * R;
        const int32_t *gs = group_start ? group_start + c0 : nullptr;
        const hipError_t e = dhmm_with_slots(NS, [&](auto ns) {
            constexpr int SLOTS = decltype(ns)::value;
            const hipError_t err = dhmm_lds_limit(dhmm_dp<SLOTS, DIR>, lds);
            if (err == hipSuccess)
                hipLaunchKernelGGL((dhmm_dp<SLOTS, DIR>), dim3((unsigned)G), dim3(64), lds, s, rc, n_states + c0, (int)c0, (int)nc,
                                   C, Smax, K, sym, len, N, T, gs, members, (int)P, score, seg, dir);
            return err;
        });
        if (e != hipSuccess) return DSP_ERR_HIP + (int)e;
    }
    return dtw_launch_status();
}

}  // namespace dsp

extern "C" size_t dsp_dhmm_workspace_bytes(int64_t C, int64_t N, int64_t P, int T, int Smax, int K)
{
    if (!dsp::dhmm_in_plan(C, N, P, T, Smax, K)) return 0;
    return dsp::dhmm_plan(C, N, P, T, Smax, K).total();
}

extern "C" int dsp_dhmm_score(const double *emit, const double *stay, const double *adv, const int32_t *n_states, int64_t C,
                              int Smax, int K, const int32_t *sym, const int32_t *len, int64_t N, int T, double *score,
                              int32_t *label, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!dsp::dhmm_in_plan(C, N, 0, T, Smax, K)) return DSP_ERR_ARGS;
    if (N == 0 || (!score && !label)) return DSP_OK;
    if (!sym || !len || (C > 0 && (!emit || !stay || !adv || !n_states))) return DSP_ERR_ARGS;
    const dsp::DhmmPlan pl = dsp::dhmm_plan(C, N, 0, T, Smax, K);
    if (!workspace || workspace_bytes < pl.total()) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double *sc = score ? score : (double *)((char *)workspace + pl.rec + pl.dir);
    if (C > 0) {
        const int rc = dsp::dhmm_run<false>(s, pl, workspace, emit, stay, adv, n_states, C, Smax, K, sym, len, N, T, nullptr,
                                            nullptr, 0, sc, nullptr);
        if (rc != DSP_OK) return rc;
    }
    if (label) hipLaunchKernelGGL(dsp::csr_label, dsp::csr_grid(N), dim3(256), 0, s, sc, N, C, label);
    return dsp::dtw_launch_status();
}

extern "C" int dsp_dhmm_align(const double *emit, const double *stay, const double *adv, const int32_t *n_states, int64_t C,
                              int Smax, int K, const int32_t *sym, const int32_t *len, int64_t N, int T,
                              const int32_t *group_start, const int32_t *members, int64_t P, double *score, int32_t *seg,
                              void *workspace, size_t workspace_bytes, void *stream)
{
    if (!dsp::dhmm_in_plan(C, N, P, T, Smax, K)) return DSP_ERR_ARGS;
    if (C == 0 || P == 0 || (!score && !seg)) return DSP_OK;
    if (!emit || !stay || !adv || !n_states || !group_start || !members || (N > 0 && (!sym || !len))) return DSP_ERR_ARGS;
    const dsp::DhmmPlan pl = dsp::dhmm_plan(C, N, P, T, Smax, K);
    if (!workspace || workspace_bytes < pl.total()) return DSP_ERR_WORKSPACE;
    if (seg)
        return dsp::dhmm_run<true>((hipStream_t)stream, pl, workspace, emit, stay, adv, n_states, C, Smax, K, sym, len, N, T,
                                   group_start, members, P, score, seg);
    return dsp::dhmm_run<false>((hipStream_t)stream, pl, workspace, emit, stay, adv, n_states, C, Smax, K, sym, len, N, T,
                                group_start, members, P, score, nullptr);
}

extern "C" int dsp_dhmm_accumulate(const int32_t *n_states, int64_t C, int Smax, int K, const int32_t *sym,
                                   const int32_t *len, int64_t N, int T, const int32_t *group_start, const int32_t *members,
                                   int64_t P, const int32_t *seg, const double *score, int32_t *cnt_emit, int32_t *cnt,
                                   int32_t *n_valid, double *total, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!dsp::dhmm_in_plan(C, N, P, T, Smax, K)) return DSP_ERR_ARGS;
    if (C == 0) return DSP_OK;
    if (!n_states || !group_start || !cnt_emit || !cnt || !n_valid || !total || (P > 0 && (!members || !seg || !score)) ||
        (N > 0 && (!sym || !len)))
        return DSP_ERR_ARGS;
    const dsp::DhmmPlan pl = dsp::dhmm_plan(C, N, P, T, Smax, K);
    if (!workspace || workspace_bytes < pl.total()) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int32_t *pmodel = (int32_t *)((char *)workspace + pl.rec + pl.dir + pl.score);
    const dim3 block(256);
    hipLaunchKernelGGL((dsp::csr_zero<int32_t, int32_t>), dsp::csr_grid(C * Smax * (int64_t)(K + 1)), block, 0, s, cnt_emit,
                       C * Smax * (int64_t)K, cnt, C * (int64_t)Smax);
    if (P > 0) {
        hipLaunchKernelGGL(dsp::dhmm_pairs, dsp::csr_grid(P), block, 0, s, n_states, C, Smax, K, sym, len, N, T, group_start,
                           members, P, seg, pmodel);
        hipLaunchKernelGGL(dsp::dhmm_count, dsp::csr_grid(P * T), block, 0, s, n_states, Smax, K, sym, len, T, members, P, seg,
                           pmodel, cnt_emit, cnt);
    }
    hipLaunchKernelGGL(dsp::dhmm_totals, dsp::csr_grid(C), block, 0, s, C, group_start, P, pmodel, score, n_valid, total);
    return dsp::dtw_launch_status();
}
