// hmm.hip -- left-to-right Gaussian hidden Markov models on the frame sequences, in the negative-log
// domain, on gfx950 (include/dsp_audiorec.h: dsp_hmm_score, dsp_hmm_align, dsp_hmm_accumulate;
// DESIGN.md §4.10).  Every value is defined bit for bit: the device sees only fp64 subtract,
// multiply, add, min and (in the re-estimation) divide in a fixed order; the logarithms are taken on
// the host when the model is built.
//
// Sequences.  float64, padded row-major, x [N, T, F] with len [N], 1 <= F <= 8, 1 <= T <= 1024 (the
// DTW plan, dtw_shape_in_plan).
// Model set.  C models padded to Smax <= 32 states, 1 <= n_states[c] <= Smax: mu, w [C, Smax, F], g,
// stay, adv [C, Smax], all float64, finite or +inf, never NaN, never -inf (the host builds them as
// w = 0.5 / var, g = 0.5 sum_f log(2 pi var_f), stay = -log p_stay, adv = -log(1 - p_stay));
// adv[c, S-1] is never read.
// Recurrence, for a sequence of length n and a model of S states:
//   e(t,s) = g[s];  for f ascending:  d = x[t,f] - mu[s,f];  e = e + w[s,f] * (d * d)    each op rounded, no FMA
//   V(0,0) = e(0,0);  V(0,s>0) = +inf
//   a = V(t-1,s) + stay[s];  b = V(t-1,s-1) + adv[s-1]   (b = +inf at s = 0)
//   V(t,s) = e(t,s) + min(a, b)
//   score  = V(n-1, S-1)     (+inf when n < S; also when n < 1, n > T, or n_states is outside 1 .. Smax)
// Path.  Walk back from (n-1, S-1): the predecessor is the advance (t-1, s-1) iff b < a strictly (ties
// stay).  Returned as seg int32 [P, Smax], seg[s] the first frame of state s: seg[0] = 0, strictly
// increasing, entries s >= S are -1; every entry of a pair whose score is +inf is -1.
// Pairs.  dsp_hmm_score: every sequence against every model, score [N, C].  dsp_hmm_align and
// dsp_hmm_accumulate: dsp_dtw_align's CSR list over the models (group_start [C + 1], members [P]); a
// members entry outside [0, N) is an invalid length and never read through.
// Re-estimation of model c from its valid members k0 < k1 < ... in list order, each with its seg
// (state s owns the frames beg = seg[s] .. end = seg[s+1] - 1, the last state up to n - 1):
//   X_k[s,f] = x[beg,f] + ... + x[end,f]      left to right; Q_k likewise over the rounded products x * x
//   accX = X_k0; accX = accX + X_k ...        list order; accQ likewise; cnt[s] = sum_k (end - beg + 1)
//   mean = accX / cnt;  var = max(accQ / cnt - mean * mean, var_floor)       each op rounded, no FMA
//   total = score_k0 + score_k1 + ...         list order; n_valid = number of valid members
// A member is valid when its index and length are, and its seg row is well formed for the model
// (seg[0] = 0, strictly increasing over the S states, seg[S-1] < n); any other member is skipped and
// nothing of it is read.  A model with no valid member or an n_states outside 1 .. Smax is copied bit
// for bit with total 0.0, n_valid 0 and cnt 0; rows s >= S of mean, var and cnt are zeros.
//
// Kernels:
//   hmm_pack   the model set as one interleaved record per state in the workspace, END-aligned to 32
//              register slots: state s of a model of S states sits in slot s + 32 - S, so the result is
//              always slot 31; the leading slots hold zeros (their cells start at +inf and stay there).
//              A record is g, stay, adv[s-1], mu[0..F), w[0..F): 2 F + 3 doubles.
//   hmm_dp<F, DIR>  one persistent wave per tile of ONE model and 64 sequences, a lane per sequence.
//              The 32 state cells of a lane live in registers, the state loop fully unrolled; the outer
//              loop runs over the frames (wave-uniform bound, the largest length of the tile; rows past
//              a lane's length compute values nothing reads).  The lane's frame comes through the vector
//              path one row ahead; the records are the same for every lane and stream through the scalar
//              path every row (a model is 32 (2 F + 3) doubles: more SGPRs than a wave has).  4 F + 4
//              fp64 instructions per cell.  DIR: one bit per cell (b < a), a compare and a carry shift;
//              a row is one 32-bit word per lane, stored [row][lane] in the wave's area of the
//              workspace; each lane then walks its own path back (hmm_internal.h's hmm_walk_back).
//              The tiles come from csr_pairs.h's csr_walk, dtw_align_dp's walk over the CSR list
//              (dsp_hmm_score's "every model against all N": the walk without a list).
//   csr_label  (csr_pairs.h) smallest score per sequence, ties to the smaller index, -1 when every
//              score is +inf.
//   hmm_pairs / hmm_sums / hmm_accumulate / hmm_finish   the re-estimation, as dba_sums /
//              dba_accumulate / dba_finish: per-pair sums in parallel, then the ordered adds with the
//              loads of 16 members issued together; csr_pairs.h's csr_zero zeroes the counts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "csr_pairs.h"
#include "dsp_audiorec.h"
#include "dtw_internal.h"
#include "hmm_internal.h"

namespace dsp {

static constexpr size_t HMM_SUMS_CAP = 128u << 20;  // bytes of X_k, Q_k and frame counts per pair chunk

// rec [C][32][2 F + 3], see above; a model with an invalid n_states gets zeros (never read)
__global__ __launch_bounds__(256) void hmm_pack(const double *__restrict__ mu, const double *__restrict__ w,
                                                const double *__restrict__ g, const double *__restrict__ stay,
                                                const double *__restrict__ adv, const int32_t *__restrict__ n_states,
                                                int64_t C, int Smax, int F, double *__restrict__ rec)
{
    const int R = 2 * F + 3;
    const int64_t total = C * HMM_SMAX * R;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int k = (int)(e % R), j = (int)((e / R) % HMM_SMAX);
        const int64_t c = e / ((int64_t)R * HMM_SMAX);
        const int S = n_states[c], s = j - (HMM_SMAX - S);
        double v = 0.0;
        if (S >= 1 && S <= Smax && s >= 0) {
            const int64_t cs = c * Smax + s;
            if (k == 0)
                v = g[cs];
            else if (k == 1)
                v = stay[cs];
            else if (k == 2)
                v = s > 0 ? adv[cs - 1] : 0.0;
            else if (k < 3 + F)
                v = mu[cs * F + (k - 3)];
            else
                v = w[cs * F + (k - 3 - F)];
        }
        rec[e] = v;
    }
}

#pragma clang fp contract(off)
// One row of the 32 slots: v holds row t-1 and is replaced by row t; xf: the lane's frame t; rec:
// the model's records (wave-uniform).  FIRST: row 0, slot j0 (state 0) starts the path.  DIR: bit j
// of word = "the predecessor of slot j is the advance" (slot 31 is shifted in first).
template <int F, bool FIRST, bool DIR>
__device__ __forceinline__ void hmm_row(double (&v)[HMM_SMAX], const double (&xf)[F], const double *__restrict__ rec,
                                        int j0, uint32_t &word)
{
    constexpr int R = 2 * F + 3;
    uint32_t md = 0;
    double cur[R];
#pragma unroll
    for (int k = 0; k < R; k++) cur[k] = rec[(HMM_SMAX - 1) * R + k];
    // slots in descending order: slot j reads row t-1 of slots j and j-1 only, so it is replaced in place
#pragma unroll
    for (int j = HMM_SMAX - 1; j >= 0; j--) {
        // the next slot's record is asked for before this slot's cell is computed; the barrier keeps
        // the scheduler from gathering the 32 records' loads (it then spills SGPRs to VGPR lanes)
        double nxt[R];
#pragma unroll
        for (int k = 0; k < R; k++) nxt[k] = j > 0 ? rec[(j - 1) * R + k] : 0.0;
        double e = cur[0];
#pragma unroll
        for (int f = 0; f < F; f++) {
            const double d = xf[f] - cur[3 + f];
            e = e + cur[3 + F + f] * (d * d);
        }
        if (FIRST) {
            v[j] = j == j0 ? e : (double)INFINITY;
        } else {
            const double a = v[j] + cur[1];
            const double b = (j > 0 ? v[j - 1] : (double)INFINITY) + cur[2];
            // md = 2 md + (b < a): the compare's bit shifted in through the carry
            if (DIR)
                asm("v_cmp_lt_f64 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(md) : "v"(b), "v"(a) : "vcc");
            v[j] = e + dtw_min(a, b);
        }
        asm volatile("" : "+v"(v[j]));  // the cell is finished here: its record's SGPRs die
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < R; k++) cur[k] = nxt[k];
    }
    if (DIR) word = md;
}

// V(n-1, S-1) of the lane's sequence xr (n its length, 0: nothing of the lane is used) under the
// model whose records are rc, state 0 in slot j0; nmax > 0 the wave's largest n.  dir: this wave's
// direction words at this lane, [row][lane]; NULL: not stored.
template <int F, bool DIR>
__device__ __forceinline__ double hmm_sweep(const double *__restrict__ rc, int j0, const double *__restrict__ xr, int n,
                                            int nmax, uint32_t *dir)
{
    double v[HMM_SMAX], xf[F];
    uint32_t word = 0;
#pragma unroll
    for (int f = 0; f < F; f++) xf[f] = xr[f];
    hmm_row<F, true, DIR>(v, xf, rc, j0, word);
    if (DIR && dir) dir[0] = 0;
    double res = n == 1 ? v[HMM_SMAX - 1] : (double)INFINITY;
    const int r1 = min(1, nmax - 1);
#pragma unroll
    for (int f = 0; f < F; f++) xf[f] = xr[(size_t)r1 * F + f];
    for (int t = 1; t < nmax; t++) {
        const int rn = min(t + 1, nmax - 1);  // the next row's loads, issued before this row's cells
        double xn[F];
#pragma unroll
        for (int f = 0; f < F; f++) xn[f] = xr[(size_t)rn * F + f];
        // the records are re-read every row: held resident they would be 64 (2 F + 3) SGPRs, and
        // hoisted out of the loop they spill.  The opaque zero keeps the loads in the loop; it is an
        // offset and not the pointer, which would lose its address space (64-lane flat loads)
        int again = 0;
        asm volatile("" : "+s"(again));
        hmm_row<F, false, DIR>(v, xf, rc + again, j0, word);
        if (DIR && dir) dir[(size_t)t * 64] = word;
        if (t == n - 1) res = v[HMM_SMAX - 1];
#pragma unroll
        for (int f = 0; f < F; f++) xf[f] = xn[f];
    }
    return res;
}
#pragma clang fp contract(on)

// The models c = 0 .. nc-1 of this launch (rec, n_states and group_start already point at the first
// one, model c0 of the set).  group_start == NULL: every model against all N sequences, the result
// of (sequence r, model c) at score[r * C + c0 + c]; else the CSR pairs, outputs indexed by p.
template <int F, bool DIR>
__global__ __launch_bounds__(64) void hmm_dp(const double *__restrict__ rec, const int32_t *__restrict__ n_states, int c0,
                                             int nc, int64_t C, int Smax, const double *__restrict__ x,
                                             const int32_t *__restrict__ len, int64_t N, int T,
                                             const int32_t *__restrict__ group_start,
                                             const int32_t *__restrict__ members, int P, double *__restrict__ score,
                                             int32_t *__restrict__ seg, uint32_t *dir_ws)
{
    constexpr int R = 2 * F + 3;
    const int lane = (int)threadIdx.x, wv = (int)blockIdx.x;
    uint32_t *dir = DIR && seg ? dir_ws + (size_t)wv * (size_t)T * 64 + lane : nullptr;
    csr_walk((int)gridDim.x, wv, nc, group_start, 0, group_start ? P : (int)N, members, len, N, T,
             [&](int cg, const CsrLane &ln) {
                 const int S = n_states[cg], n = ln.len;
                 const bool sok = S >= 1 && S <= Smax;
                 const double *__restrict__ rc = rec + (size_t)cg * HMM_SMAX * R;
                 const int64_t p = ln.p;
                 double res = INFINITY;
                 if (sok && ln.lmax > 0)
                     res = hmm_sweep<F, DIR>(rc, HMM_SMAX - S, x + (int64_t)ln.row * T * F, n, ln.lmax, dir);
                 if (!ln.inr) return;
                 if (score) score[group_start ? p : p * C + c0 + cg] = res;
                 if (DIR && seg) hmm_walk_back(dir, n, S, HMM_SMAX, Smax, res < INFINITY, seg + p * Smax);
             });
}

// ---- re-estimation ----
// A thread per pair of [p_lo, p_hi): its model (the group that holds p) and whether it is valid;
// plen [p - p_lo][s] = frames of state s, all 0 for a pair that is skipped.
__global__ __launch_bounds__(256) void hmm_pairs(const int32_t *__restrict__ n_states, int64_t C, int Smax,
                                                 const int32_t *__restrict__ len, int64_t N, int T,
                                                 const int32_t *__restrict__ group_start,
                                                 const int32_t *__restrict__ members, int p_lo, int p_hi,
                                                 const int32_t *__restrict__ seg, int32_t *__restrict__ plen)
{
    for (int64_t p = p_lo + (int64_t)blockIdx.x * 256 + threadIdx.x; p < p_hi; p += (int64_t)gridDim.x * 256) {
        const int64_t lo = csr_group_of(group_start, C, p);
        const int S = n_states[lo], mem = members[p];
        const int32_t *__restrict__ ps = seg + p * Smax;
        int32_t *__restrict__ pl = plen + (p - p_lo) * Smax;
        bool ok = S >= 1 && S <= Smax && mem >= 0 && mem < N && p >= group_start[lo] && p < group_start[lo + 1];
        const int n = ok ? len[mem] : 0;
        ok = ok && n >= 1 && n <= T && hmm_seg_ok(ps, S, n);
        for (int s = 0; s < Smax; s++) pl[s] = ok && s < S ? (s + 1 < S ? ps[s + 1] : n) - ps[s] : 0;
    }
}

#pragma clang fp contract(off)
// X_k and Q_k, a thread per (pair, state, channel) of [p_lo, p_hi): the state's frames added left to right
__global__ __launch_bounds__(256) void hmm_sums(const double *__restrict__ x, int T, int F, int Smax,
                                                const int32_t *__restrict__ members, int p_lo, int p_hi,
                                                const int32_t *__restrict__ seg, const int32_t *__restrict__ plen,
                                                double *__restrict__ sx, double *__restrict__ sq)
{
    const int64_t total = (int64_t)(p_hi - p_lo) * Smax * F;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int f = (int)(e % F);
        const int64_t row = e / F, p = p_lo + row / Smax;  // row = (pair - p_lo) * Smax + s
        const int cnt = plen[row];
        if (cnt <= 0) continue;
        const int beg = seg[p * Smax + row % Smax];
        const double *__restrict__ s = x + ((int64_t)members[p] * T + beg) * F + f;
        double sum = s[0], sqs = s[0] * s[0];
        for (int j = 1; j < cnt; j++) {
            const double v = s[(int64_t)j * F];
            sum = sum + v;
            sqs = sqs + v * v;
        }
        sx[e] = sum;
        sq[e] = sqs;
    }
}

// One thread per (model c, state s, channel f): acc = acc + X_k over the pairs of [p_lo, p_hi) in list
// order (plen, sx, sq indexed by p - p_lo).  accx / accq (the mean and var outputs), cnt, n_valid and
// total carry the sums from one pair chunk to the next; cnt == 0: no valid member seen yet.
__global__ __launch_bounds__(256) void hmm_accumulate(int F, int Smax, const int32_t *__restrict__ n_states, int64_t C,
                                                      const int32_t *__restrict__ group_start, int p_lo, int p_hi,
                                                      const int32_t *__restrict__ plen, const double *__restrict__ sx,
                                                      const double *__restrict__ sq, const double *__restrict__ score,
                                                      double *__restrict__ accx, double *__restrict__ accq,
                                                      int32_t *__restrict__ cnt, int32_t *__restrict__ n_valid,
                                                      double *__restrict__ total_out)
{
    const int64_t total = C * Smax * F;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int f = (int)(e % F), s = (int)((e / F) % Smax);
        const int64_t c = e / ((int64_t)F * Smax);
        const int S = n_states[c];
        if (S < 1 || S > Smax || s >= S) continue;
        const int g0 = clampi(group_start[c], p_lo, p_hi), g1 = clampi(group_start[c + 1], p_lo, p_hi);
        const bool lead = s == 0 && f == 0;
        int count = cnt[e], nv = lead ? n_valid[c] : 0;
        double ax = accx[e], aq = accq[e], tot = lead ? total_out[c] : 0.0;
        for (int p0 = g0; p0 < g1; p0 += HMM_BATCH) {
            int l[HMM_BATCH];
            double vx[HMM_BATCH], vq[HMM_BATCH], sc[HMM_BATCH];
#pragma unroll
            for (int u = 0; u < HMM_BATCH; u++) {
                const bool in_group = p0 + u < g1;
                const int64_t row = (int64_t)(p0 + u - p_lo) * Smax + s;
                l[u] = in_group ? plen[row] : 0;
                vx[u] = in_group ? sx[row * F + f] : 0.0;  // not written for a skipped pair, not used then
                vq[u] = in_group ? sq[row * F + f] : 0.0;
                sc[u] = lead && in_group ? score[p0 + u] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < HMM_BATCH; u++) {
                if (l[u] <= 0) continue;
                ax = count == 0 ? vx[u] : ax + vx[u];
                aq = count == 0 ? vq[u] : aq + vq[u];
                if (lead) {
                    tot = count == 0 ? sc[u] : tot + sc[u];
                    nv++;
                }
                count += l[u];
            }
        }
        accx[e] = ax;
        accq[e] = aq;
        cnt[e] = count;
        if (lead) {
            n_valid[c] = nv;
            total_out[c] = tot;
        }
    }
}

// mean and var from the sums, zeros behind the model's states; the previous model where nothing was summed
__global__ __launch_bounds__(256) void hmm_finish(const double *__restrict__ mu_prev, const double *__restrict__ var_prev,
                                                  const int32_t *__restrict__ n_states, int64_t C, int Smax, int F,
                                                  const int32_t *__restrict__ cnt, const int32_t *__restrict__ n_valid,
                                                  double var_floor, double *__restrict__ mean, double *__restrict__ var,
                                                  int32_t *__restrict__ cnt_out, double *__restrict__ total_out)
{
    const int64_t total = C * Smax * F;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int f = (int)(e % F), s = (int)((e / F) % Smax);
        const int64_t c = e / ((int64_t)F * Smax);
        const int S = n_states[c];
        const bool summed = S >= 1 && S <= Smax && n_valid[c] > 0;
        double m = 0.0, q = 0.0;
        int k = 0;
        if (!summed) {
            m = mu_prev[e];
            q = var_prev[e];
        } else if (s < S) {
            k = cnt[e];
            m = mean[e] / (double)k;
            const double d = var[e] / (double)k - m * m;
            q = (d > var_floor || d != d) ? d : var_floor;
        }
        mean[e] = m;
        var[e] = q;
        if (f == 0) cnt_out[e / F] = k;
        if (!summed && s == 0 && f == 0) total_out[c] = 0.0;
    }
}
#pragma clang fp contract(on)

// ---- host side ----
static bool hmm_in_plan(int64_t C, int64_t N, int64_t P, int T, int F, int Smax)
{
    return C >= 0 && C <= HMM_CMAX && N >= 0 && N < 0x7fffffff && P >= 0 && P < 0x7fffffff && Smax >= 1 &&
           Smax <= HMM_SMAX && dtw_shape_in_plan(T, T, F);
}

// workspace: [records of the C models][direction words of G waves][score [N, C], for labels without
// scores][frame counts, X_k and Q_k of one pair chunk and the counts of the C models: dsp_hmm_accumulate]
struct HmmPlan {
    int64_t pc;
    int G;
    size_t rec, dir, score, plen, sums, cnt;
    size_t total() const { return rec + dir + score + plen + 2 * sums + cnt; }
};
static HmmPlan hmm_plan(int64_t C, int64_t N, int64_t P, int T, int F, int Smax)
{
    HmmPlan pl;
    pl.pc = std::max<int64_t>(1, std::min<int64_t>(P, (int64_t)(HMM_SUMS_CAP / ((size_t)Smax * (4 + 16 * F)))));
    pl.G = csr_waves(P / 64 + std::min<int64_t>(C, HMM_GCHUNK), hmm_dir_bytes(T));
    pl.rec = up256((size_t)C * HMM_SMAX * (2 * F + 3) * 8);
    pl.dir = up256(pl.G * hmm_dir_bytes(T));
    pl.score = up256((size_t)N * C * 8);
    pl.plen = up256((size_t)pl.pc * Smax * 4);
    pl.sums = up256((size_t)pl.pc * Smax * F * 8);
    pl.cnt = up256((size_t)C * Smax * F * 4);
    return pl;
}

// hmm_dp<F, DIR> as DTW_LAUNCH_F wants it: a template of F alone
template <int F>
static constexpr auto hmm_dp_score = hmm_dp<F, false>;
template <int F>
static constexpr auto hmm_dp_align = hmm_dp<F, true>;

// the records, then the DP over all models in launches of at most HMM_GCHUNK; tiles: of the whole call
template <bool DIR>
static int hmm_run(hipStream_t s, const HmmPlan &pl, void *ws, const double *mu, const double *w, const double *g,
                   const double *stay, const double *adv, const int32_t *n_states, int64_t C, int Smax, const double *x,
                   const int32_t *len, int64_t N, int T, int F, const int32_t *group_start, const int32_t *members,
                   int64_t P, double *score, int32_t *seg)
{
    double *rec = (double *)ws;
    uint32_t *dir = (uint32_t *)((char *)ws + pl.rec);
    const int R = 2 * F + 3;
    hipLaunchKernelGGL(hmm_pack, csr_grid(C * HMM_SMAX * R), dim3(256), 0, s, mu, w, g, stay, adv, n_states, C, Smax, F, rec);
    for (int64_t c0 = 0; c0 < C; c0 += HMM_GCHUNK) {
        const int64_t nc = std::min<int64_t>(HMM_GCHUNK, C - c0);
        const int64_t tiles = group_start ? P / 64 + nc : nc * ((N + 63) / 64);
        const int G = DIR ? std::min(pl.G, csr_waves(tiles, hmm_dir_bytes(T))) : csr_waves(tiles, 0);
        const double *rc = rec + (size_t)c0 * HMM_SMAX * R;
        const int32_t *gs = group_start ? group_start + c0 : nullptr;
        if (DIR) {
            DTW_LAUNCH_F(F, hmm_dp_align, dim3((unsigned)G), dim3(64), 0, s, rc, n_states + c0, (int)c0, (int)nc, C, Smax, x,
                         len, N, T, gs, members, (int)P, score, seg, dir)
        } else {
            DTW_LAUNCH_F(F, hmm_dp_score, dim3((unsigned)G), dim3(64), 0, s, rc, n_states + c0, (int)c0, (int)nc, C, Smax, x,
                         len, N, T, gs, members, (int)P, score, seg, dir)
        }
    }
    return dsp::dtw_launch_status();
}

}  // namespace dsp

extern "C" size_t dsp_hmm_workspace_bytes(int64_t C, int64_t N, int64_t P, int T, int F, int Smax)
{
    if (!dsp::hmm_in_plan(C, N, P, T, F, Smax)) return 0;
    return dsp::hmm_plan(C, N, P, T, F, Smax).total();
}

extern "C" int dsp_hmm_score(const double *mu, const double *w, const double *g, const double *stay, const double *adv,
                             const int32_t *n_states, int64_t C, int Smax, const double *x, const int32_t *len, int64_t N,
                             int T, int F, double *score, int32_t *label, void *workspace, size_t workspace_bytes,
                             void *stream)
{
    if (!dsp::hmm_in_plan(C, N, 0, T, F, Smax)) return DSP_ERR_ARGS;
    if (N == 0 || (!score && !label)) return DSP_OK;
    if (!x || !len || (C > 0 && (!mu || !w || !g || !stay || !adv || !n_states))) return DSP_ERR_ARGS;
    const dsp::HmmPlan pl = dsp::hmm_plan(C, N, 0, T, F, Smax);
    if (!workspace || workspace_bytes < pl.total()) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double *sc = score ? score : (double *)((char *)workspace + pl.rec + pl.dir);
    if (C > 0) {
        const int rc = dsp::hmm_run<false>(s, pl, workspace, mu, w, g, stay, adv, n_states, C, Smax, x, len, N, T, F,
                                           nullptr, nullptr, 0, sc, nullptr);
        if (rc != DSP_OK) return rc;
    }
    if (label) hipLaunchKernelGGL(dsp::csr_label, dsp::csr_grid(N), dim3(256), 0, s, sc, N, C, label);
    return dsp::dtw_launch_status();
}

extern "C" int dsp_hmm_align(const double *mu, const double *w, const double *g, const double *stay, const double *adv,
                             const int32_t *n_states, int64_t C, int Smax, const double *x, const int32_t *len, int64_t N,
                             int T, int F, const int32_t *group_start, const int32_t *members, int64_t P, double *score,
                             int32_t *seg, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!dsp::hmm_in_plan(C, N, P, T, F, Smax)) return DSP_ERR_ARGS;
    if (C == 0 || P == 0 || (!score && !seg)) return DSP_OK;
    if (!mu || !w || !g || !stay || !adv || !n_states || !group_start || !members || (N > 0 && (!x || !len)))
        return DSP_ERR_ARGS;
    const dsp::HmmPlan pl = dsp::hmm_plan(C, N, P, T, F, Smax);
    if (!workspace || workspace_bytes < pl.total()) return DSP_ERR_WORKSPACE;
    if (seg)
        return dsp::hmm_run<true>((hipStream_t)stream, pl, workspace, mu, w, g, stay, adv, n_states, C, Smax, x, len, N, T,
                                  F, group_start, members, P, score, seg);
    return dsp::hmm_run<false>((hipStream_t)stream, pl, workspace, mu, w, g, stay, adv, n_states, C, Smax, x, len, N, T, F,
                               group_start, members, P, score, nullptr);
}

extern "C" int dsp_hmm_accumulate(const double *mu_prev, const double *var_prev, const int32_t *n_states, int64_t C,
                                  int Smax, const double *x, const int32_t *len, int64_t N, int T, int F,
                                  const int32_t *group_start, const int32_t *members, int64_t P, const int32_t *seg,
                                  const double *score, double var_floor, double *mean, double *var, int32_t *cnt,
                                  int32_t *n_valid, double *total, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!dsp::hmm_in_plan(C, N, P, T, F, Smax) || !(var_floor == var_floor)) return DSP_ERR_ARGS;
    if (C == 0) return DSP_OK;
    if (!mu_prev || !var_prev || !n_states || !group_start || !mean || !var || !cnt || !n_valid || !total ||
        mean == mu_prev || var == var_prev || (P > 0 && (!members || !seg || !score)) || (N > 0 && (!x || !len)))
        return DSP_ERR_ARGS;
    const dsp::HmmPlan pl = dsp::hmm_plan(C, N, P, T, F, Smax);
    if (!workspace || workspace_bytes < pl.total()) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *wsp = (char *)workspace + pl.rec + pl.dir + pl.score;
    int32_t *plen = (int32_t *)wsp;
    double *sx = (double *)(wsp + pl.plen), *sq = (double *)(wsp + pl.plen + pl.sums);
    int32_t *cntf = (int32_t *)(wsp + pl.plen + 2 * pl.sums);
    const int64_t elems = C * Smax * F;
    const dim3 block(256);
    hipLaunchKernelGGL((dsp::csr_zero<int32_t, int32_t>), dsp::csr_grid(elems + C), block, 0, s, cntf, elems, n_valid, C);
    for (int64_t p_lo = 0; p_lo < P; p_lo += pl.pc) {
        const int64_t p_hi = std::min(P, p_lo + pl.pc), np = p_hi - p_lo;
        hipLaunchKernelGGL(dsp::hmm_pairs, dsp::csr_grid(np), block, 0, s, n_states, C, Smax, len, N, T, group_start,
                           members, (int)p_lo, (int)p_hi, seg, plen);
        hipLaunchKernelGGL(dsp::hmm_sums, dsp::csr_grid(np * Smax * F), block, 0, s, x, T, F, Smax, members, (int)p_lo,
                           (int)p_hi, seg, plen, sx, sq);
        hipLaunchKernelGGL(dsp::hmm_accumulate, dsp::csr_grid(elems), block, 0, s, F, Smax, n_states, C, group_start,
                           (int)p_lo, (int)p_hi, plen, sx, sq, score, mean, var, cntf, n_valid, total);
    }
    hipLaunchKernelGGL(dsp::hmm_finish, dsp::csr_grid(elems), block, 0, s, mu_prev, var_prev, n_states, C, Smax, F, cntf,
                       n_valid, var_floor, mean, var, cnt, total);
    return dsp::dtw_launch_status();
}
