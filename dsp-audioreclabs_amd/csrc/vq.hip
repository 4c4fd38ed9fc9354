// vq.hip -- vector-quantisation codebooks on the frame sequences, on gfx950 (include/dsp_audiorec.h:
// dsp_vq_score, dsp_vq_assign, dsp_vq_accumulate).  Every value is defined bit for bit:
// the device sees only fp64 subtract, multiply, add, compare and (in the re-estimation) one divide, in
// a fixed order, each operation rounded, never fused.
//
// Sequences.  float64, padded row-major, x [N, T, F] with len [N], 1 <= F <= 8, 1 <= T <= 1024 (the
// DTW plan, dtw_shape_in_plan).
// Codebook set.  C <= 2^20 codebooks padded to Kmax <= 256 codewords: cb [C, Kmax, F] float64, n_codes
// int32 [C], 1 <= n_codes[c] <= Kmax.  Frames and codewords are finite (for other values the results are
// unspecified, but nothing is read or written out of bounds); rows k >= n_codes[c] are never read by the
// search.
// For frame t of a sequence of n frames and a codebook of K codewords:
//   d(t,k) = e0 * e0, then for f = 1 .. F-1 ascending:  e = x[t,f] - cb[k,f];  d = d + e * e    (e0 = x[t,0] - cb[k,0])
//   best = d(t,0), code = 0;  for k = 1 .. K-1 ascending:  if d(t,k) < best (strictly): best = d(t,k), code = k
//   D = best(0);  D = D + best(t)  for t = 1 .. n-1 ascending
// Ties go to the smaller codeword index; D is the sequence's total distortion.  D is +inf, and every
// code -1, when n < 1, n > T, n_codes[c] is outside 1 .. Kmax, or a list entry is outside [0, N); nothing
// of such a member is read through.  A distance that overflows is +inf; if all overflow the code is 0.
// Pairs.  dsp_vq_score: every sequence against every codebook, score [N, C].  dsp_vq_assign and
// dsp_vq_accumulate: dsp_dtw_align's CSR list over the codebooks (group_start [C + 1], members [P]).
// Re-estimation of codebook c from a GIVEN code [P, T] and dist [P].  A member is valid when its index
// and length are, and every code[p, t], t < n, lies in [0, n_codes[c]); other members are skipped and
// nothing of their frames is read.  With the valid members k0 < k1 < ... in list order:
//   m_k[j]    = number of the member's frames with code j
//   X_k[j,f]  = the member's frames with code j added left to right (t ascending; the first is the value itself)
//   accX[j,f] = X_k of the first member with m_k[j] > 0, then accX + X_k for each later member with m_k[j] > 0
//               (a member with m_k[j] = 0 adds nothing to cell j, not even 0.0: a cell of -0.0 frames stays -0.0)
//   cnt[j]    = sum_k m_k[j];   centroid[j,f] = accX[j,f] / (double)cnt[j] where cnt[j] > 0, cb_prev[c,j,f] where not
//   total[c]  = dist_k0 + dist_k1 + ...  in list order;   n_valid[c] = number of valid members
// Rows j >= K of centroid and cnt are zeros.  A codebook with no valid member or an n_codes outside
// 1 .. Kmax is copied bit for bit (all Kmax rows) with total 0.0, n_valid 0 and cnt 0.
//
// Kernels:
//   vq_search<F, CODES>  one persistent wave per tile of ONE codebook and 64 sequences, a lane per
//              sequence (csr_pairs.h's csr_walk; dsp_vq_score is the walk without a list).  The tile's
//              codebook is staged into LDS (at most 256 x 8 doubles = 16 KiB, padded to a multiple of 4
//              codewords with NaN, which no compare ever selects) when it differs from the one the wave
//              staged last, and read with wave-uniform addresses (a broadcast: no bank conflict).  The
//              outer loop runs over the frames (wave-uniform bound, the largest length of the tile; rows
//              past a lane's length compute values nothing reads), the lane's frame arriving one row
//              ahead through the vector path.  The codeword loop is unrolled by 4: four independent
//              distance chains of 3 F - 1 fp64 instructions, then four compares, each with the selects
//              of best and code.  CODES: the lane's code of a row goes to an LDS tile [16 rows][64 lanes],
//              which the wave writes out transposed every 16 rows: 16 consecutive int32 of one pair's row
//              of code [P, T] per 16 lanes (64 contiguous bytes), not 64 scattered words per row.
//   csr_label  (csr_pairs.h) the argmin of dsp_vq_score.
//   vq_pairs / vq_sums / vq_accumulate / vq_finish   the re-estimation, as hmm_pairs / hmm_sums /
//              hmm_accumulate / hmm_finish: per-pair validity and per-cell frame counts, per-pair cell
//              sums in parallel, then the ordered adds in list order with the loads of 16 members issued
//              together, then the divide and the copy rule; pairs in chunks whose sums and counts fit
//              128 MiB, csr_pairs.h's csr_zero before the first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "csr_pairs.h"
#include "dsp_audiorec.h"
#include "dtw_internal.h"

namespace dsp {

static constexpr int VQ_KMAX = 256;                     // codewords of one codebook at most (16 KiB of LDS at F = 8)
static constexpr int64_t VQ_CMAX = 1 << 20;             // codebooks in a set at most
static constexpr int VQ_GCHUNK = 1024;                  // codebooks per launch at most (a wave walks their group_start)
static constexpr int VQ_UNROLL = 4;                     // codewords whose distance chains run side by side
static constexpr int VQ_ROWS = 16;                      // rows of codes gathered in LDS before a write-out
static constexpr int VQ_RSTRIDE = 66;                   // words per gathered row: conflict-free both ways
static constexpr size_t VQ_SUMS_CAP = 128u << 20;       // bytes of X_k, m_k and validity per pair chunk
static constexpr int VQ_BATCH = 16;                     // members whose loads an accumulate thread keeps in flight

#pragma clang fp contract(off)
// best and code of the lane's frame xf among the kp (a multiple of VQ_UNROLL) staged codewords.  Starting
// from +inf with code 0 is the definition's "best = d(t,0), code = 0": d(t,0) replaces +inf unless it is
// +inf itself.  The NaN rows behind the codebook's last codeword never compare below best.
template <int F>
__device__ __forceinline__ void vq_nearest(const double *cbs, int kp, const double (&xf)[F], double &best, int &code)
{
    best = INFINITY;
    code = 0;
#pragma unroll 1
    for (int k0 = 0; k0 < kp; k0 += VQ_UNROLL) {
        double d[VQ_UNROLL];
#pragma unroll
        for (int u = 0; u < VQ_UNROLL; u++) {
            const double *q = cbs + (k0 + u) * F;
            double e = xf[0] - q[0];
            double s = e * e;
#pragma unroll
            for (int f = 1; f < F; f++) {
                e = xf[f] - q[f];
                s = s + e * e;
            }
            d[u] = s;
        }
#pragma unroll
        for (int u = 0; u < VQ_UNROLL; u++) {
            const bool lt = d[u] < best;
            best = lt ? d[u] : best;
            code = lt ? k0 + u : code;
        }
    }
}

// The codebooks c = 0 .. nc-1 of this launch (cb, n_codes and group_start already point at the first
// one, codebook c0 of the set).  group_start == NULL: every codebook against all N sequences, the result
// of (sequence r, codebook c) at out[r * C + c0 + c]; else the CSR pairs, outputs indexed by p.
template <int F, bool CODES>
__global__ __launch_bounds__(64) void vq_search(const double *__restrict__ cb, const int32_t *__restrict__ n_codes, int c0,
                                                int nc, int64_t C, int Kmax, const double *__restrict__ x,
                                                const int32_t *__restrict__ len, int64_t N, int T,
                                                const int32_t *__restrict__ group_start,
                                                const int32_t *__restrict__ members, int P, double *__restrict__ out,
                                                int32_t *__restrict__ code)
{
    __shared__ double cbs[VQ_KMAX * F];
    __shared__ int32_t cds[CODES ? VQ_ROWS * VQ_RSTRIDE : 1];
    const int lane = (int)threadIdx.x, wv = (int)blockIdx.x;
    int staged = -1;
    csr_walk((int)gridDim.x, wv, nc, group_start, 0, group_start ? P : (int)N, members, len, N, T,
             [&](int cg, const CsrLane &ln) {
                 const int K = n_codes[cg];
                 const bool kok = K >= 1 && K <= Kmax;
                 const int n = kok ? ln.len : 0, rows = kok ? ln.lmax : 0;  // rows: wave-uniform
                 const int kp = (K + VQ_UNROLL - 1) & ~(VQ_UNROLL - 1);      // <= VQ_KMAX, a multiple of VQ_UNROLL
                 const int64_t p = ln.p;
                 if (rows > 0 && staged != cg) {
                     __syncthreads();
                     const double *__restrict__ src = cb + (size_t)cg * Kmax * F;
                     for (int e = lane; e < kp * F; e += 64) cbs[e] = e < K * F ? src[e] : __builtin_nan("");
                     __syncthreads();
                     staged = cg;
                 }
                 // the tile's pairs are consecutive: lane l holds pair p - lane + l, the first ninr are inside the group
                 const int ninr = CODES ? __popcll(__ballot(ln.inr)) : 0;
                 int32_t *__restrict__ crow = CODES && code ? code + (p - lane) * T : nullptr;
                 double D = INFINITY;
                 if (rows > 0) {
                     const double *__restrict__ xr = x + (int64_t)ln.row * T * F;
                     double xf[F];
#pragma unroll
                     for (int f = 0; f < F; f++) xf[f] = xr[f];
                     for (int t = 0; t < rows; t++) {
                         const int rn = min(t + 1, rows - 1);  // the next row's loads, issued before this row's codewords
                         double xn[F];
#pragma unroll
                         for (int f = 0; f < F; f++) xn[f] = xr[(size_t)rn * F + f];
                         double best;
                         int bc;
                         vq_nearest<F>(cbs, kp, xf, best, bc);
                         D = t == 0 ? best : (t < n ? D + best : D);
                         if (CODES && crow) {
                             const int r = t & (VQ_ROWS - 1);
                             cds[r * VQ_RSTRIDE + lane] = t < n ? bc : -1;
                             if (r == VQ_ROWS - 1 || t == rows - 1) {
                                 // rows t - r .. t of the 64 pairs, 16 lanes per pair: 64 contiguous bytes each
                                 __syncthreads();
                                 const int col = lane & (VQ_ROWS - 1);
#pragma unroll 4
                                 for (int j = 0; j < 64 / 4; j++) {
                                     const int s = j * 4 + (lane >> 4);
                                     if (s < ninr && col <= r) crow[(int64_t)s * T + (t - r) + col] = cds[col * VQ_RSTRIDE + s];
                                 }
                                 __syncthreads();
                             }
                         }
#pragma unroll
                         for (int f = 0; f < F; f++) xf[f] = xn[f];
                     }
                     if (n == 0) D = INFINITY;
                 }
                 if (CODES && crow)  // behind the tile's longest sequence (everything for an invalid codebook)
                     for (int s = 0; s < ninr; s++)
                         for (int i = rows + lane; i < T; i += 64) crow[(int64_t)s * T + i] = -1;
                 if (ln.inr && out) out[group_start ? p : p * C + c0 + cg] = D;
             });
}
#pragma clang fp contract(on)

// ---- re-estimation ----
// A thread per pair of [p_lo, p_hi): its codebook (the group that holds p, by bisection of group_start)
// and whether it is valid (pok); pcnt [p - p_lo][j] = its frames with code j, all 0 for a pair that is skipped.
__global__ __launch_bounds__(256) void vq_pairs(const int32_t *__restrict__ n_codes, int64_t C, int Kmax,
                                                const int32_t *__restrict__ len, int64_t N, int T,
                                                const int32_t *__restrict__ group_start,
                                                const int32_t *__restrict__ members, int p_lo, int p_hi,
                                                const int32_t *__restrict__ code, int32_t *__restrict__ pcnt,
                                                int32_t *__restrict__ pok)
{
    for (int64_t p = p_lo + (int64_t)blockIdx.x * 256 + threadIdx.x; p < p_hi; p += (int64_t)gridDim.x * 256) {
        int64_t lo = 0, hi = C;  // the last c with group_start[c] <= p
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) / 2;
            if (group_start[mid] <= p)
                lo = mid;
            else
                hi = mid;
        }
        const int K = n_codes[lo], mem = members[p];
        const int32_t *__restrict__ pc = code + p * T;
        int32_t *__restrict__ pm = pcnt + (p - p_lo) * Kmax;
        bool ok = K >= 1 && K <= Kmax && mem >= 0 && mem < N && group_start[lo] <= p && p < group_start[lo + 1];
        const int n = ok ? len[mem] : 0;
        ok = ok && n >= 1 && n <= T;
        for (int t = 0; ok && t < n; t++) ok = pc[t] >= 0 && pc[t] < K;
        for (int j = 0; j < Kmax; j++) pm[j] = 0;
        for (int t = 0; ok && t < n; t++) pm[pc[t]]++;
        pok[p - p_lo] = ok ? 1 : 0;
    }
}

#pragma clang fp contract(off)
// X_k, a thread per (pair, cell, channel) of [p_lo, p_hi): the member's frames with the cell's code added
// left to right
__global__ __launch_bounds__(256) void vq_sums(const double *__restrict__ x, const int32_t *__restrict__ len, int T, int F,
                                               int Kmax, const int32_t *__restrict__ members, int p_lo, int p_hi,
                                               const int32_t *__restrict__ code, const int32_t *__restrict__ pcnt,
                                               double *__restrict__ sx)
{
    const int64_t total = (int64_t)(p_hi - p_lo) * Kmax * F;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int f = (int)(e % F);
        const int64_t row = e / F, p = p_lo + row / Kmax;  // row = (pair - p_lo) * Kmax + j
        const int j = (int)(row % Kmax);
        int left = pcnt[row];
        if (left <= 0) continue;
        const int mem = members[p];  // valid: the pair has frames counted
        const int32_t *__restrict__ pc = code + p * T;
        const double *__restrict__ s = x + (int64_t)mem * T * F + f;
        const int n = len[mem];
        double sum = 0.0;
        bool first = true;
        for (int t = 0; t < n && left > 0; t++) {
            if (pc[t] != j) continue;
            const double v = s[(int64_t)t * F];
            sum = first ? v : sum + v;
            first = false;
            left--;
        }
        sx[e] = sum;
    }
}

// One thread per (codebook c, cell j, channel f): acc = acc + X_k over the pairs of [p_lo, p_hi) in list
// order (pcnt, pok, sx indexed by p - p_lo).  accx (the centroid output), cnt, n_valid and total carry the
// sums from one pair chunk to the next; cnt == 0: no frame of the cell seen yet, n_valid == 0: no valid
// member seen yet.
__global__ __launch_bounds__(256) void vq_accumulate(int F, int Kmax, const int32_t *__restrict__ n_codes, int64_t C,
                                                     const int32_t *__restrict__ group_start, int p_lo, int p_hi,
                                                     const int32_t *__restrict__ pcnt, const int32_t *__restrict__ pok,
                                                     const double *__restrict__ sx, const double *__restrict__ dist,
                                                     double *__restrict__ accx, int32_t *__restrict__ cnt,
                                                     int32_t *__restrict__ n_valid, double *__restrict__ total_out)
{
    const int64_t total = C * Kmax * F;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int f = (int)(e % F), j = (int)((e / F) % Kmax);
        const int64_t c = e / ((int64_t)F * Kmax);
        const int K = n_codes[c];
        if (K < 1 || K > Kmax || j >= K) continue;
        const int g0 = clampi(group_start[c], p_lo, p_hi), g1 = clampi(group_start[c + 1], p_lo, p_hi);
        const bool lead = j == 0 && f == 0;
        int count = cnt[e], nv = lead ? n_valid[c] : 0;
        double ax = accx[e], tot = lead ? total_out[c] : 0.0;
        for (int p0 = g0; p0 < g1; p0 += VQ_BATCH) {
            int l[VQ_BATCH], ok[VQ_BATCH];
            double vx[VQ_BATCH], sc[VQ_BATCH];
#pragma unroll
            for (int u = 0; u < VQ_BATCH; u++) {
                const bool in_group = p0 + u < g1;
                const int64_t row = (int64_t)(p0 + u - p_lo) * Kmax + j;
                l[u] = in_group ? pcnt[row] : 0;
                vx[u] = in_group ? sx[row * F + f] : 0.0;  // not written for an empty cell, not used then
                ok[u] = lead && in_group ? pok[p0 + u - p_lo] : 0;
                sc[u] = lead && in_group ? dist[p0 + u] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < VQ_BATCH; u++) {
                if (ok[u]) {
                    tot = nv == 0 ? sc[u] : tot + sc[u];
                    nv++;
                }
                if (l[u] <= 0) continue;
                ax = count == 0 ? vx[u] : ax + vx[u];
                count += l[u];
            }
        }
        accx[e] = ax;
        cnt[e] = count;
        if (lead) {
            n_valid[c] = nv;
            total_out[c] = tot;
        }
    }
}

// the centroids from the sums, zeros behind the codebook's codewords; the previous codeword where a cell
// got no frame, the previous codebook where nothing was summed
__global__ __launch_bounds__(256) void vq_finish(const double *__restrict__ cb_prev, const int32_t *__restrict__ n_codes,
                                                 int64_t C, int Kmax, int F, const int32_t *__restrict__ cnt,
                                                 const int32_t *__restrict__ n_valid, double *__restrict__ centroid,
                                                 int32_t *__restrict__ cnt_out, double *__restrict__ total_out)
{
    const int64_t total = C * Kmax * F;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int f = (int)(e % F), j = (int)((e / F) % Kmax);
        const int64_t c = e / ((int64_t)F * Kmax);
        const int K = n_codes[c];
        const bool summed = K >= 1 && K <= Kmax && n_valid[c] > 0;
        double m = 0.0;
        int k = 0;
        if (!summed) {
            m = cb_prev[e];
        } else if (j < K) {
            k = cnt[e];
            m = k > 0 ? centroid[e] / (double)k : cb_prev[e];
        }
        centroid[e] = m;
        if (f == 0) cnt_out[e / F] = k;
        if (!summed && j == 0 && f == 0) total_out[c] = 0.0;
    }
}
#pragma clang fp contract(on)

// ---- host side ----
static bool vq_in_plan(int64_t C, int64_t N, int64_t P, int T, int F, int Kmax)
{
    return C >= 0 && C <= VQ_CMAX && N >= 0 && N < 0x7fffffff && P >= 0 && P < 0x7fffffff && Kmax >= 1 &&
           Kmax <= VQ_KMAX && dtw_shape_in_plan(T, T, F);
}

// workspace: [score [N, C], for labels without scores][frame counts, validity and X_k of one pair chunk
// and the counts of the C codebooks: dsp_vq_accumulate]
struct VqPlan {
    int64_t pc;
    size_t score, pcnt, pok, sums, cnt;
    size_t total() const { return score + pcnt + pok + sums + cnt; }
};
static VqPlan vq_plan(int64_t C, int64_t N, int64_t P, int T, int F, int Kmax)
{
    VqPlan pl;
    pl.pc = std::max<int64_t>(1, std::min<int64_t>(P, (int64_t)(VQ_SUMS_CAP / ((size_t)Kmax * (4 + 8 * F) + 4))));
    pl.score = up256((size_t)N * C * 8);
    pl.pcnt = up256((size_t)pl.pc * Kmax * 4);
    pl.pok = up256((size_t)pl.pc * 4);
    pl.sums = up256((size_t)pl.pc * Kmax * F * 8);
    pl.cnt = up256((size_t)C * Kmax * F * 4);
    return pl;
}

// vq_search<F, CODES> as DTW_LAUNCH_F wants it: a template of F alone
template <int F>
static constexpr auto vq_search_dist = vq_search<F, false>;
template <int F>
static constexpr auto vq_search_codes = vq_search<F, true>;

// the search over all codebooks in launches of at most VQ_GCHUNK
template <bool CODES>
static int vq_run(hipStream_t s, const double *cb, const int32_t *n_codes, int64_t C, int Kmax, const double *x,
                  const int32_t *len, int64_t N, int T, int F, const int32_t *group_start, const int32_t *members,
                  int64_t P, double *out, int32_t *code)
{
    for (int64_t c0 = 0; c0 < C; c0 += VQ_GCHUNK) {
        const int64_t nc = std::min<int64_t>(VQ_GCHUNK, C - c0);
        const int64_t tiles = group_start ? P / 64 + nc : nc * ((N + 63) / 64);
        const int G = (int)std::max<int64_t>(1, std::min<int64_t>(tiles, DTW_WAVES));
        const double *cbc = cb + (size_t)c0 * Kmax * F;
        const int32_t *gs = group_start ? group_start + c0 : nullptr;
        if (CODES) {
            DTW_LAUNCH_F(F, vq_search_codes, dim3((unsigned)G), dim3(64), 0, s, cbc, n_codes + c0, (int)c0, (int)nc, C, Kmax, x,
                         len, N, T, gs, members, (int)P, out, code)
        } else {
            DTW_LAUNCH_F(F, vq_search_dist, dim3((unsigned)G), dim3(64), 0, s, cbc, n_codes + c0, (int)c0, (int)nc, C, Kmax, x,
                         len, N, T, gs, members, (int)P, out, code)
        }
    }
    return dsp::dtw_launch_status();
}

}  // namespace dsp

extern "C" size_t dsp_vq_workspace_bytes(int64_t C, int64_t N, int64_t P, int T, int F, int Kmax)
{
    if (!dsp::vq_in_plan(C, N, P, T, F, Kmax)) return 0;
    return dsp::vq_plan(C, N, P, T, F, Kmax).total();
}

extern "C" int dsp_vq_score(const double *cb, const int32_t *n_codes, int64_t C, int Kmax, const double *x,
                            const int32_t *len, int64_t N, int T, int F, double *score, int32_t *label, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    if (!dsp::vq_in_plan(C, N, 0, T, F, Kmax)) return DSP_ERR_ARGS;
    if (N == 0 || (!score && !label)) return DSP_OK;
    if (!x || !len || (C > 0 && (!cb || !n_codes))) return DSP_ERR_ARGS;
    const dsp::VqPlan pl = dsp::vq_plan(C, N, 0, T, F, Kmax);
    if (!workspace || workspace_bytes < pl.total()) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double *sc = score ? score : (double *)workspace;
    if (C > 0) {
        const int rc = dsp::vq_run<false>(s, cb, n_codes, C, Kmax, x, len, N, T, F, nullptr, nullptr, 0, sc, nullptr);
        if (rc != DSP_OK) return rc;
    }
    if (label) hipLaunchKernelGGL(dsp::csr_label, dsp::csr_grid(N), dim3(256), 0, s, sc, N, C, label);
    return dsp::dtw_launch_status();
}

extern "C" int dsp_vq_assign(const double *cb, const int32_t *n_codes, int64_t C, int Kmax, const double *x,
                             const int32_t *len, int64_t N, int T, int F, const int32_t *group_start,
                             const int32_t *members, int64_t P, double *dist, int32_t *code, void *workspace,
                             size_t workspace_bytes, void *stream)
{
    if (!dsp::vq_in_plan(C, N, P, T, F, Kmax)) return DSP_ERR_ARGS;
    if (C == 0 || P == 0 || (!dist && !code)) return DSP_OK;
    if (!cb || !n_codes || !group_start || !members || (N > 0 && (!x || !len))) return DSP_ERR_ARGS;
    const dsp::VqPlan pl = dsp::vq_plan(C, N, P, T, F, Kmax);
    if (!workspace || workspace_bytes < pl.total()) return DSP_ERR_WORKSPACE;
    if (code)
        return dsp::vq_run<true>((hipStream_t)stream, cb, n_codes, C, Kmax, x, len, N, T, F, group_start, members, P, dist,
                                 code);
    return dsp::vq_run<false>((hipStream_t)stream, cb, n_codes, C, Kmax, x, len, N, T, F, group_start, members, P, dist,
                              nullptr);
}

extern "C" int dsp_vq_accumulate(const double *cb_prev, const int32_t *n_codes, int64_t C, int Kmax, const double *x,
                                 const int32_t *len, int64_t N, int T, int F, const int32_t *group_start,
                                 const int32_t *members, int64_t P, const int32_t *code, const double *dist,
                                 double *centroid, int32_t *cnt, int32_t *n_valid, double *total, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    if (!dsp::vq_in_plan(C, N, P, T, F, Kmax)) return DSP_ERR_ARGS;
    if (C == 0) return DSP_OK;
    if (!cb_prev || !n_codes || !group_start || !centroid || !cnt || !n_valid || !total || centroid == cb_prev ||
        (P > 0 && (!members || !code || !dist)) || (N > 0 && (!x || !len)))
        return DSP_ERR_ARGS;
    const dsp::VqPlan pl = dsp::vq_plan(C, N, P, T, F, Kmax);
    if (!workspace || workspace_bytes < pl.total()) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *wsp = (char *)workspace + pl.score;
    int32_t *pcnt = (int32_t *)wsp, *pok = (int32_t *)(wsp + pl.pcnt);
    double *sx = (double *)(wsp + pl.pcnt + pl.pok);
    int32_t *cntf = (int32_t *)(wsp + pl.pcnt + pl.pok + pl.sums);
    const int64_t elems = C * Kmax * F;
    const dim3 block(256);
    hipLaunchKernelGGL((dsp::csr_zero<int32_t, int32_t>), dsp::csr_grid(elems + C), block, 0, s, cntf, elems, n_valid, C);
    for (int64_t p_lo = 0; p_lo < P; p_lo += pl.pc) {
        const int64_t p_hi = std::min(P, p_lo + pl.pc), np = p_hi - p_lo;
        hipLaunchKernelGGL(dsp::vq_pairs, dsp::csr_grid(np), block, 0, s, n_codes, C, Kmax, len, N, T, group_start, members,
                           (int)p_lo, (int)p_hi, code, pcnt, pok);
        hipLaunchKernelGGL(dsp::vq_sums, dsp::csr_grid(np * Kmax * F), block, 0, s, x, len, T, F, Kmax, members, (int)p_lo,
                           (int)p_hi, code, pcnt, sx);
        hipLaunchKernelGGL(dsp::vq_accumulate, dsp::csr_grid(elems), block, 0, s, F, Kmax, n_codes, C, group_start, (int)p_lo,
                           (int)p_hi, pcnt, pok, sx, dist, centroid, cntf, n_valid, total);
    }
    hipLaunchKernelGGL(dsp::vq_finish, dsp::csr_grid(elems), block, 0, s, cb_prev, n_codes, C, Kmax, F, cntf, n_valid,
                       centroid, cnt, total);
    return dsp::dtw_launch_status();
}
