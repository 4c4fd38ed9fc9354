// dtw_align.hip -- the warping path of dynamic time warping and one DTW barycentre averaging (DBA)
// update on it, on gfx950 (include/dsp_audiorec.h: dsp_dtw_align, dsp_dtw_dba_update).
// c, D, the band and invalid lengths are dtw.hip's, unchanged.
//
// Path.  For a pair with lengths n (side a, index i) and m (side b, index j), walk back from
// (n-1, m-1) to (0, 0): the predecessor of (i, j) is the FIRST of (i-1, j-1), (i-1, j), (i, j-1)
// whose D equals the minimum of the three, neighbours outside the grid or the band counting as
// +inf.  D is defined bit for bit, so the path is.  The tie rule is stated in a / b indices and is
// not symmetric: this kernel walks the grid transposed (a along the register strip) and names its
// neighbours accordingly -- "left" in the strip is (i-1, j), the row above is (i, j-1).
// Ranges.  From a's side, two int32 rows per pair: frame i of a is matched to frames lo[i] .. hi[i]
// of b; lo[0] = 0, hi[n-1] = m-1, hi[i] <= lo[i+1] <= hi[i] + 1, and the path's cells are exactly
// {(i, j): lo[i] <= j <= hi[i]}.  Entries i >= n are -1; a pair with an invalid length on either
// side (or a members entry outside [0, Nb)) has dist = +inf and every entry -1.
// Pairs.  A CSR list over a: the sequences aligned to a[c] are b[members[p]] for p in
// [group_start[c], group_start[c+1]); outputs are indexed by p.
// One DBA update, template c of length L, valid members k0 < k1 < ... in list order:
//   S_k[i,f] = s_k[lo,f] + s_k[lo+1,f] + ... + s_k[hi,f]      left to right, each sum rounded
//   acc[i,f] = S_k0[i,f];  acc = acc + S_k for k1, k2, ...    in list order
//   cnt[i]   = sum_k (hi - lo + 1)                            integer
//   new[i,f] = acc[i,f] / (double)cnt[i]                      one rounded division
//   inertia  = D_k0(end);  inertia = inertia + D_k(end)       (dtw^2, before the sqrt) in list order
// Rows i >= L of the output are zeros; a template whose own length is invalid or that has no valid
// member is copied bit for bit with inertia 0.0.
//
// Kernels:
//   dtw_align_dp<F>  one wave per tile of 64 members of ONE group: dtw_internal.h's sweep with DIR,
//              the group's a sequence as the uniform side and a lane per member.  Beyond D each
//              cell yields two bits (does D(i-1, j-1), does D(i-1, j) equal the minimum: the rule's
//              first two candidates -- the sweep's diagonal and its "left"); the 2 x 32 bits of a
//              strip row are one 64-bit word per lane, stored [strip][row][lane] -- one coalesced
//              512-byte store per row, nothing per cell.
//              After the tile's strips each lane walks its own path back through those words (at
//              most n + m - 1 steps; a word is re-read only when the strip or the row changes) and
//              writes lo / hi.  The walk clamps at i = 0 and j = 0, so it ends and stays inside the
//              pair's words whatever the codes hold.  Waves are persistent: csr_pairs.h's csr_walk
//              (shared with hmm.hip) gives wave w of G the tiles w, w + G, ... of the launch's groups
//              (at most 1024 per launch), so the words and the edges are per wave and bounded
//              whatever P is.
//   dba_sums   a thread per (pair, frame, channel): S_k from the pair's ranges, all pairs in parallel.
//   dba_accumulate / dba_finish   a thread per (template, frame, channel): acc = acc + S_k over the
//              chunk's pairs in list order, then the division; csr_pairs.h's csr_zero zeroes
//              the counts first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "csr_pairs.h"
#include "dsp_audiorec.h"
#include "dtw_internal.h"

namespace dsp {

static constexpr size_t DTW_ALIGN_WAVE_CAP = 1024u << 20;  // bytes of code words and edges per launch
static constexpr size_t DTW_ALIGN_RANGE_CAP = 128u << 20;  // bytes of lo, hi and S_k per DBA pair chunk
static constexpr int DTW_ALIGN_GCHUNK = 1024;              // groups per launch at most
static constexpr int DBA_BATCH = 16;                       // members whose loads a DBA thread keeps in flight

// The groups c = 0 .. nc-1 of this launch (apad, len_a and group_start already point at the first
// one) and of their pairs those in [p_lo, p_hi).  dist is indexed by p; d2 (D(end) before the sqrt),
// lo and hi by p - p_lo.  Any of dist, d2 and the lo / hi pair may be NULL.
template <int F>
__global__ __launch_bounds__(64) void dtw_align_dp(const double *__restrict__ apad, const int32_t *__restrict__ len_a,
                                                   const int32_t *__restrict__ group_start, int nc, int Ta,
                                                   const double *__restrict__ b, const int32_t *__restrict__ len_b,
                                                   int64_t Nb, int Tb, const int32_t *__restrict__ members, int p_lo,
                                                   int p_hi, int window, double *__restrict__ dist,
                                                   double *__restrict__ d2, int32_t *__restrict__ lo,
                                                   int32_t *__restrict__ hi, double *__restrict__ edge_ws,
                                                   unsigned long long *dir_ws)
{
    const int lane = (int)threadIdx.x, wv = (int)blockIdx.x;
    const int smax = (Ta + DTW_STRIP - 1) / DTW_STRIP;
    double *__restrict__ edge = edge_ws + (size_t)wv * (size_t)Tb * 64 + lane;
    unsigned long long *dir = dir_ws + (size_t)wv * (size_t)smax * (size_t)Tb * 64 + lane;  // [strip][row][lane]
    csr_walk(
        (int)gridDim.x, wv, nc, group_start, p_lo, p_hi, members, len_b, Nb, Tb, [&](int cg, const CsrLane &ln) {
            const int n = len_a[cg], m = ln.len;
            const bool nok = n >= 1 && n <= Ta;
            const double *__restrict__ q = apad + ((int64_t)cg * (Ta + DTW_STRIP) + DTW_STRIP) * F;  // frame 0
            const int S = nok ? (n + DTW_STRIP - 1) / DTW_STRIP : 0;
            const int64_t p = ln.p;
            double res = INFINITY;
            if (nok && ln.lmax > 0)
                res = dtw_sweep<F, true>(q, b + (int64_t)ln.row * Tb * F, n, m, ln.lmax, window, Tb, edge,
                                         lo ? dir : nullptr);
            if (!ln.inr) return;
            if (dist) dist[p] = res < INFINITY ? sqrt(res) : (double)INFINITY;
            if (d2) d2[p - p_lo] = res;
            if (!lo) return;
            int32_t *__restrict__ plo = lo + (p - p_lo) * Ta, *__restrict__ phi = hi + (p - p_lo) * Ta;
            int filled = 0;
            if (nok && m > 0) {
                // the lane's own walk back; cell (i, j) sits in strip S-1 - (n-1-i)/32 at bit
                // (n-1-i)%32 of both halves of row j's word (the strip's last cell was shifted in last)
                int i = n - 1, j = m - 1, ks = -1, kr = -1;
                unsigned long long word = 0;
                phi[i] = j;
                while (i > 0 || j > 0) {
                    const int k = n - 1 - i, s = S - 1 - (k >> 5), bit = k & 31;
                    if (s != ks || j != kr) {
                        word = dir[((size_t)s * Tb + j) * 64];
                        ks = s;
                        kr = j;
                    }
                    int code = ((word >> bit) & 1) ? 0 : (((word >> (32 + bit)) & 1) ? 1 : 2);
                    if (i == 0)
                        code = 2;
                    else if (j == 0)
                        code = 1;
                    if (code == 2) {
                        j--;
                    } else {
                        plo[i] = j;
                        i--;
                        if (code == 0) j--;
                        phi[i] = j;
                    }
                }
                plo[0] = 0;
                filled = n;
            }
            for (int i = filled; i < Ta; i++) {
                plo[i] = -1;
                phi[i] = -1;
            }
        });
}

#pragma clang fp contract(off)
// S_k of the launch's groups' pairs in [p_lo, p_hi) -- one run of pairs, the list being CSR: only
// their ranges were written -- a thread per (pair, frame i, channel f): the member's frames lo .. hi
// added left to right into sums [pair - p_lo][i][f].  A pair with an invalid length has lo = -1 and
// nothing of it is read; rows behind the template's length hold -1 as well.  (A group_start that is
// not non-decreasing breaks the "one run" and leaves rows nobody wrote: the range and the member are
// checked against the sequence's bounds, so such a list gives wrong sums but reads nothing outside.)
__global__ __launch_bounds__(256) void dba_sums(const double *__restrict__ seqs, int64_t N, int Ts, int F, int Tt,
                                                const int32_t *__restrict__ group_start, int nc,
                                                const int32_t *__restrict__ members, int p_lo, int p_hi,
                                                const int32_t *__restrict__ lo, const int32_t *__restrict__ hi,
                                                double *__restrict__ sums)
{
    const int q_lo = clampi(group_start[0], p_lo, p_hi), q_hi = clampi(group_start[nc], p_lo, p_hi);
    const int64_t first = (int64_t)(q_lo - p_lo) * Tt * F, total = (int64_t)(q_hi - p_lo) * Tt * F;
    for (int64_t e = first + (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int f = (int)(e % F);
        const int64_t row = e / F;  // (pair - p_lo) * Tt + i
        const int l = lo[row];
        if (l < 0) continue;
        const int h = hi[row], mem = members[p_lo + row / Tt];
        if (h < l || h >= Ts || mem < 0 || mem >= N) continue;
        const double *__restrict__ s = seqs + (int64_t)mem * Ts * F + f;
        double sum = s[(int64_t)l * F];
        for (int j = l + 1; j <= h; j++) sum = sum + s[(int64_t)j * F];
        sums[e] = sum;
    }
}

// One thread per (template c, frame i, channel f) of the launch's groups: acc = acc + S_k over the
// pairs of [p_lo, p_hi) in list order (lo, hi, sums, d2 indexed by p - p_lo).  acc (the output
// templates), cnt and inertia carry the sums from one pair chunk to the next; cnt == 0: no valid
// member seen yet.  The loads of DBA_BATCH members are issued together (none depends on another);
// the additions stay in list order.
__global__ __launch_bounds__(256) void dba_accumulate(int F, const int32_t *__restrict__ group_start, int nc, int Tt,
                                                      const int32_t *__restrict__ len_t, int p_lo, int p_hi,
                                                      const int32_t *__restrict__ lo, const int32_t *__restrict__ hi,
                                                      const double *__restrict__ sums,
                                                      const double *__restrict__ d2, double *__restrict__ acc,
                                                      int32_t *__restrict__ cnt, double *__restrict__ inertia)
{
    const int64_t total = (int64_t)nc * Tt * F;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int f = (int)(e % F), i = (int)((e / F) % Tt), c = (int)(e / ((int64_t)F * Tt));
        const int L = len_t[c];
        if (L < 1 || L > Tt || i >= L) continue;
        const int g0 = clampi(group_start[c], p_lo, p_hi), g1 = clampi(group_start[c + 1], p_lo, p_hi);
        const bool lead = i == 0 && f == 0 && inertia;
        int count = cnt[e];
        double a = acc[e], in = lead ? inertia[c] : 0.0;
        for (int p0 = g0; p0 < g1; p0 += DBA_BATCH) {
            int l[DBA_BATCH], h[DBA_BATCH];
            double sum[DBA_BATCH], dd[DBA_BATCH];
#pragma unroll
            for (int u = 0; u < DBA_BATCH; u++) {
                const bool in_group = p0 + u < g1;
                const int64_t row = (int64_t)(p0 + u - p_lo) * Tt + i;
                l[u] = in_group ? lo[row] : -1;
                h[u] = in_group ? hi[row] : -1;
                sum[u] = in_group ? sums[row * F + f] : 0.0;  // not written for an invalid pair, not used then
                dd[u] = lead && in_group ? d2[p0 + u - p_lo] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < DBA_BATCH; u++) {
                if (l[u] < 0) continue;
                a = count == 0 ? sum[u] : a + sum[u];
                if (lead) in = count == 0 ? dd[u] : in + dd[u];
                count += h[u] - l[u] + 1;
            }
        }
        acc[e] = a;
        cnt[e] = count;
        if (lead) inertia[c] = in;
    }
}

// acc / cnt, zeros behind the template's length; the template itself where nothing was summed
__global__ __launch_bounds__(256) void dba_finish(const double *__restrict__ tmpl, const int32_t *__restrict__ len_t,
                                                  int nc, int Tt, int F, const int32_t *__restrict__ cnt,
                                                  double *__restrict__ out, double *__restrict__ inertia)
{
    const int64_t total = (int64_t)nc * Tt * F;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int f = (int)(e % F), i = (int)((e / F) % Tt), c = (int)(e / ((int64_t)F * Tt));
        const int L = len_t[c];
        const bool summed = L >= 1 && L <= Tt && cnt[(int64_t)c * Tt * F] > 0;
        out[e] = !summed ? tmpl[e] : (i < L ? out[e] / (double)cnt[e] : 0.0);
        if (!summed && i == 0 && f == 0 && inertia) inertia[c] = 0.0;
    }
}
#pragma clang fp contract(on)

// ---- host side ----
static bool align_in_plan(int64_t Na, int64_t Nb, int64_t P, int Ta, int Tb, int F)
{
    return Na >= 0 && Na < 0x7fffffff && Nb >= 0 && Nb <= 0x7fffffff && P >= 0 && P <= 0x7fffffff &&
           dtw_shape_in_plan(Ta, Tb, F);
}
// a wave's code words [strips][Tb][64], and with them its edge column [Tb][64]
static size_t align_dir_bytes(int Ta, int Tb) { return (size_t)((Ta + DTW_STRIP - 1) / DTW_STRIP) * Tb * 64 * 8; }
static size_t align_wave_bytes(int Ta, int Tb) { return align_dir_bytes(Ta, Tb) + (size_t)Tb * 64 * 8; }
// waves of a launch over nc groups and np pairs: no more than its tiles can be
static int align_waves(int64_t nc, int64_t np, int Ta, int Tb)
{
    const int64_t cap = std::max<int64_t>(1, (int64_t)(DTW_ALIGN_WAVE_CAP / align_wave_bytes(Ta, Tb)));
    return (int)std::max<int64_t>(1, std::min<int64_t>(np / 64 + nc, std::min<int64_t>(DTW_WAVES, cap)));
}
static int64_t align_pair_chunk(int64_t P, int Ta, int F)
{
    return std::max<int64_t>(1, std::min<int64_t>(P, (int64_t)(DTW_ALIGN_RANGE_CAP / ((size_t)Ta * (8 + 8 * F)))));
}

// workspace: [code words and edges of G waves][padded a of one group chunk][lo, hi, S_k, d2 of one
// pair chunk and cnt of one group chunk: dsp_dtw_dba_update only]
struct AlignPlan {
    int64_t nc, pc;
    int G;
    size_t waves, pad, ranges, sums, d2, cnt;
    size_t total() const { return waves + pad + 2 * ranges + sums + d2 + cnt; }
};
static AlignPlan align_plan(int64_t Na, int64_t P, int Ta, int Tb, int F)
{
    AlignPlan pl;
    pl.nc = std::max<int64_t>(1, std::min<int64_t>(Na, DTW_ALIGN_GCHUNK));
    pl.pc = align_pair_chunk(P, Ta, F);
    pl.G = align_waves(pl.nc, P, Ta, Tb);
    pl.waves = up256((size_t)pl.G * align_wave_bytes(Ta, Tb));
    pl.pad = dtw_pad_bytes(pl.nc, Ta, F);
    pl.ranges = up256((size_t)pl.pc * Ta * 4);
    pl.sums = up256((size_t)pl.pc * Ta * F * 8);
    pl.d2 = up256((size_t)pl.pc * 8);
    pl.cnt = up256((size_t)pl.nc * Ta * F * 4);
    return pl;
}

// nc groups from group c0 on, their pairs in [p_lo, p_hi): the padded copy (pad = true), then the DP
static int align_launch(hipStream_t s, const AlignPlan &pl, void *ws, bool pad, const double *a, const int32_t *len_a,
                        int64_t c0, int64_t nc, int Ta, const double *b, const int32_t *len_b, int64_t Nb, int Tb,
                        int F, int window, const int32_t *group_start, const int32_t *members, int64_t p_lo,
                        int64_t p_hi, double *dist, double *d2, int32_t *lo, int32_t *hi)
{
    unsigned long long *dir = (unsigned long long *)ws;
    double *edge = (double *)((char *)ws + (size_t)pl.G * align_dir_bytes(Ta, Tb));
    double *apad = (double *)((char *)ws + pl.waves);
    if (pad) dtw_launch_pad(s, a + c0 * Ta * F, nc, Ta, F, apad);
    const int G = std::min(pl.G, align_waves(nc, p_hi - p_lo, Ta, Tb));
    DTW_LAUNCH_F(F, dtw_align_dp, dim3((unsigned)G), dim3(64), 0, s, apad, len_a + c0, group_start + c0, (int)nc, Ta, b,
                 len_b, Nb, Tb, members, (int)p_lo, (int)p_hi, window, dist, d2, lo, hi, edge, dir)
    return dtw_launch_status();
}

}  // namespace dsp

extern "C" size_t dsp_dtw_align_workspace_bytes(int64_t Na, int64_t P, int Ta, int Tb, int F)
{
    if (!dsp::align_in_plan(Na, 0, P, Ta, Tb, F)) return 0;
    return dsp::align_plan(Na, P, Ta, Tb, F).total();
}

extern "C" int dsp_dtw_align(const double *a, const int32_t *len_a, int64_t Na, int Ta, const double *b,
                             const int32_t *len_b, int64_t Nb, int Tb, int F, int window,
                             const int32_t *group_start, const int32_t *members, int64_t P, double *dist, int32_t *lo,
                             int32_t *hi, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!dsp::align_in_plan(Na, Nb, P, Ta, Tb, F) || (lo == nullptr) != (hi == nullptr)) return DSP_ERR_ARGS;
    if (Na == 0 || P == 0 || (!dist && !lo)) return DSP_OK;
    if (!a || !len_a || !group_start || !members || (Nb > 0 && (!b || !len_b))) return DSP_ERR_ARGS;
    const dsp::AlignPlan pl = dsp::align_plan(Na, P, Ta, Tb, F);
    if (!workspace || workspace_bytes < pl.total()) return DSP_ERR_WORKSPACE;
    for (int64_t c0 = 0; c0 < Na; c0 += pl.nc) {
        const int rc = dsp::align_launch((hipStream_t)stream, pl, workspace, true, a, len_a, c0,
                                         std::min(pl.nc, Na - c0), Ta, b, len_b, Nb, Tb, F, window, group_start,
                                         members, 0, P, dist, nullptr, lo, hi);
        if (rc != DSP_OK) return rc;
    }
    return DSP_OK;
}

extern "C" int dsp_dtw_dba_update(const double *tmpl, const int32_t *len_t, int64_t C, int Tt, const double *seqs,
                                  const int32_t *len_s, int64_t N, int Ts, int F, int window,
                                  const int32_t *group_start, const int32_t *members, int64_t P, double *tmpl_out,
                                  double *inertia, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!dsp::align_in_plan(C, N, P, Tt, Ts, F)) return DSP_ERR_ARGS;
    if (C == 0) return DSP_OK;
    if (!tmpl || !len_t || !tmpl_out || tmpl_out == tmpl || !group_start || (P > 0 && !members) ||
        (N > 0 && (!seqs || !len_s)))
        return DSP_ERR_ARGS;
    const dsp::AlignPlan pl = dsp::align_plan(C, P, Tt, Ts, F);
    if (!workspace || workspace_bytes < pl.total()) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)workspace + pl.waves + pl.pad;
    int32_t *lo = (int32_t *)w, *hi = (int32_t *)(w + pl.ranges);
    double *sums = (double *)(w + 2 * pl.ranges), *d2 = (double *)(w + 2 * pl.ranges + pl.sums);
    int32_t *cnt = (int32_t *)(w + 2 * pl.ranges + pl.sums + pl.d2);
    for (int64_t c0 = 0; c0 < C; c0 += pl.nc) {
        const int64_t nc = std::min(pl.nc, C - c0), elems = nc * Tt * F;
        const dim3 grid = dsp::csr_grid(elems), block(256);
        double *out = tmpl_out + c0 * Tt * F, *in = inertia ? inertia + c0 : nullptr;
        hipLaunchKernelGGL((dsp::csr_zero<int32_t, int32_t>), grid, block, 0, s, cnt, elems, nullptr, 0);
        for (int64_t p_lo = 0; p_lo < P; p_lo += pl.pc) {
            const int64_t p_hi = std::min(P, p_lo + pl.pc);
            const int rc = dsp::align_launch(s, pl, workspace, p_lo == 0, tmpl, len_t, c0, nc, Tt, seqs, len_s, N, Ts,
                                             F, window, group_start, members, p_lo, p_hi, nullptr, d2, lo, hi);
            if (rc != DSP_OK) return rc;
            hipLaunchKernelGGL(dsp::dba_sums, dsp::csr_grid((p_hi - p_lo) * Tt * F), block, 0, s, seqs, N, Ts, F, Tt,
                               group_start + c0, (int)nc, members, (int)p_lo, (int)p_hi, lo, hi, sums);
            hipLaunchKernelGGL(dsp::dba_accumulate, grid, block, 0, s, F, group_start + c0, (int)nc, Tt, len_t + c0,
                               (int)p_lo, (int)p_hi, lo, hi, sums, d2, out, cnt, in);
        }
        hipLaunchKernelGGL(dsp::dba_finish, grid, block, 0, s, tmpl + c0 * Tt * F, len_t + c0, (int)nc, Tt, F, cnt, out,
                           in);
        const int rc = dsp::dtw_launch_status();
        if (rc != DSP_OK) return rc;
    }
    return DSP_OK;
}
