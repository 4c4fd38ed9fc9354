// dhmm_fb.hip -- the forward algorithm (evaluation) and the forward-backward expected counts (Baum-Welch
// training) of the discrete-observation HMMs of dhmm.hip, in the SCALED PROBABILITY domain, on gfx950
// (include/dsp_audiorec.h: dsp_dhmm_forward, dsp_dhmm_expect).  An extension like
// §4.8-§4.15: nothing here restates a reference file.  Every row of the trellis is rescaled by a power of
// two taken from the row's own maximum, so the device needs only fp64 multiply, add, max, frexp and ldexp
// and one IEEE division per frame: every value is defined bit for bit, and the device takes no logarithm
// -- the likelihood leaves it as a (mantissa, exponent) pair and the host takes the one log.
//
// Symbols.  sym int32 [N, T] with len int32 [N], 1 <= T <= 1024, as in dsp_dhmm_score.  Alphabet: K <= 256.
// Probability model set.  C models padded to Smax <= 32 states: pemit float64 [C, Smax, K], pstay, padv
// float64 [C, Smax], n_states int32 [C].  Every entry read is 0.0 or lies in [2^-300, 1], never NaN;
// padv[c, S-1] and the rows s >= S are never read.
// Arithmetic.  Every operation rounded to fp64, products formed as written, nothing fused (fp contract
// off), fp64 denormals kept.  B = pemit, a = pstay, d = padv, o = the symbol row.
// Forward, a model of S states and a sequence of n frames:
//   u_0(0) = B[0,o_0];  u_0(s>0) = 0
//   u_t(s) = (A_{t-1}(s)*a[s] + A_{t-1}(s-1)*d[s-1]) * B[s,o_t]     (the second product is 0.0 at s = 0)
//   m_t = max_s u_t(s)
//     m_t > 0:  k_t = frexp exponent of m_t (m_t = f * 2^k_t, 0.5 <= f < 1);
//               A_t(s) = ldexp(u_t(s), -k_t);  E_t = E_{t-1} + k_t     (E_{-1} = 0)
//     m_t == 0: A_t = u_t (all zeros);  E_t = E_{t-1}
//   v = A_{n-1}(S-1);  v == 0: (mant, expo) = (0.0, 0), "zero likelihood";
//   else (f, k) = frexp(v): mant = f in [0.5, 1), expo = E_{n-1} + k (int32)
// The likelihood of ending in the last state is mant * 2^expo.  It is zero when n < S (from the
// recurrence), when n < 1 or n > T, when n_states is outside 1 .. Smax, for a list entry outside [0, N),
// and when any sym[t], t < n, is outside [0, K): such a symbol never indexes the table (the index is
// clamped and the result forced).  Label: the model of the largest likelihood, decided exactly -- the
// larger expo, then the larger mant, ties to the smaller index; -1 when every likelihood is zero.
// Backward:
//   Bh_{n-1}(S-1) = 1;  Bh_{n-1}(s < S-1) = 0
//   w_t(s) = a[s]*(B[s,o_{t+1}]*Bh_{t+1}(s)) + d[s]*(B[s+1,o_{t+1}]*Bh_{t+1}(s+1))   (second term 0.0 at s = S-1)
//   each row rescaled by its own maximum's exponent as above (a zero row stays zero); no exponent kept.
// Posteriors:
//   g_t(s) = A_t(s) * Bh_t(s);  D_t = g_t(0) + g_t(1) + ... + g_t(S-1) (ascending s);  r_t = 1.0 / D_t;
//   gamma_t(s) = g_t(s) * r_t
// A member is valid when its index and length are, all its symbols at t < n lie in [0, K), its model's
// n_states is valid and every D_t, 0 <= t < n, is > 0 with a finite reciprocal r_t (a positive D_t below
// about 2^-1024, a subnormal, has r_t = +inf: no 0 * inf is ever formed); any other member is skipped whole,
// so gamma, occ_emit and n_valid hold finite values only.
// Expected counts: G_p[s,k] = the gamma_t(s) of the frames with o_t = k added in DESCENDING t from 0.0;
// occ_emit[c,s,k] = the G_p[s,k] of the valid members added in list order from 0.0; rows s >= S and models
// without a valid member are zeros; n_valid[c] counts the valid members.
//
// Kernels (dhmm_dp's shape, dhmm.hip; the record, its pack kernel and its staging are hmm_internal.h's -- the
// padding slots hold 0.0, here zero probabilities: their cells are 0.0, which no maximum and no sum sees, so
// the bits do not depend on NS):
//   dhmm_fwd<NS>  one persistent wave per tile of ONE model and 64 sequences (csr_walk), a lane per
//              sequence, the NS cells in registers, the lane's symbol one row ahead.  A cell is 3 multiplies,
//              1 add, 1 max and 1 ldexp; a row adds one frexp exponent.  Nothing is kept per row.
//   dhmm_fb<NS>   the same forward sweep storing the A rows [row][slot][lane] in the wave's own area of the
//              workspace (the slots in front of the model's states are wave-uniform zeros and are not
//              stored), then the backward sweep with Bh in registers: it reads the A rows back, forms D_t,
//              r_t and gamma, and adds gamma into the pair's OWN table G_p [K][NS] in the workspace --
//              plain load, add, store: the lane owns its pair.  Descending t is the sweep's own order.
//   dhmm_fb_sum   the list-order add: a thread per (model, symbol, slot), the loads of 16 members issued
//              together, skipped pairs contributing nothing, the sums carried in occ_emit from one pair
//              chunk to the next (the pairs are chunked so the G_p tables stay inside DHMM_GP_CAP bytes).
//   dhmm_fb_label the exact comparison of the (mant, expo) pairs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "csr_pairs.h"
#include "dsp_audiorec.h"
#include "dtw_internal.h"
#include "hmm_internal.h"

namespace dsp {

// max of two values that are never NaN, as the one instruction it is (dtw_min's reason)
__device__ __forceinline__ double dfb_max(double x, double y)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
    return r;
}

#pragma clang fp contract(off)
// The row's rescale: v = ldexp(v, -k), k the frexp exponent of the row's maximum (0 for a zero row); returns k
template <int NS>
__device__ __forceinline__ int dfb_rescale(double (&v)[NS])
{
    double m = v[0];
#pragma unroll
    for (int j = 1; j < NS; j++) m = dfb_max(m, v[j]);
    const int k = m > 0.0 ? __builtin_amdgcn_frexp_exp(m) : 0;
#pragma unroll
    for (int j = 0; j < NS; j++) v[j] = __builtin_ldexp(v[j], -k);
    return k;
}

// One forward row before its rescale: v holds A_{t-1} and is replaced by u_t; erow: the slots of the lane's
// own symbol in LDS; tr: (stay, adv[s-1]) per slot in LDS.  FIRST: row 0, slot j0 (state 0) starts.
template <int NS, bool FIRST>
__device__ __forceinline__ void dfb_fwd_row(double (&v)[NS], const double2 *erow, const double2 *tr, int j0)
{
    double2 e2[NS / 2];
#pragma unroll
    for (int i = NS / 2 - 1; i >= 0; i--) e2[i] = erow[i];
    // slots in descending order: slot j reads row t-1 of slots j and j-1 only, so it is replaced in place
#pragma unroll
    for (int j = NS - 1; j >= 0; j--) {
        const double e = (j & 1) ? e2[j / 2].y : e2[j / 2].x;
        if (FIRST) {
            v[j] = j == j0 ? e : 0.0;
        } else {
            const double2 sa = tr[j];
            const double a = v[j] * sa.x;
            const double b = j > 0 ? v[j - 1] * sa.y : 0.0;
            v[j] = (a + b) * e;
        }
    }
}

// The forward pass of the lane's symbol row sr (n its length, 0: nothing of the lane is used) under the
// model staged in LDS, state 0 in slot j0; nmax > 0 the wave's largest n.  (mant, expo) as defined above.
// rows: this wave's A rows at this lane, [row][slot][lane]; STORE: the slots j >= j0 of every row are kept.
template <int NS, bool STORE>
__device__ __forceinline__ void dfb_forward(const unsigned char *tab, const double2 *tr, int j0, int K,
                                            const int32_t *__restrict__ sr, int n, int nmax, double *rows, double &mant,
                                            int &expo)
{
    double v[NS];
    auto row_of = [&](int k) { return (const double2 *)(tab + (unsigned)min((unsigned)k, (unsigned)(K - 1)) * dhmm_pitch(NS)); };
    auto keep = [&](int t) {
#pragma unroll
        for (int j = 0; j < NS; j++)
            if (j >= j0) rows[((size_t)t * NS + j) * 64] = v[j];
    };
    int k = sr[0];
    bool bad = n < 1 || (unsigned)k >= (unsigned)K;
    dfb_fwd_row<NS, true>(v, row_of(k), tr, j0);
    int E = dfb_rescale<NS>(v);
    if (STORE) keep(0);
    double resv = n == 1 ? v[NS - 1] : 0.0;
    int resE = E;
    k = sr[min(1, nmax - 1)];
    for (int t = 1; t < nmax; t++) {
        const int kn = sr[min(t + 1, nmax - 1)];  // the next row's symbol, asked for before this row's cells
        bad = bad || (t < n && (unsigned)k >= (unsigned)K);
        dfb_fwd_row<NS, false>(v, row_of(k), tr, j0);
        E += dfb_rescale<NS>(v);
        if (STORE) keep(t);
        if (t == n - 1) {
            resv = v[NS - 1];
            resE = E;
        }
        k = kn;
    }
    const bool some = !bad && resv > 0.0;
    mant = some ? __builtin_amdgcn_frexp_mant(resv) : 0.0;
    expo = some ? resE + __builtin_amdgcn_frexp_exp(resv) : 0;
}

// The backward pass and the posteriors of a lane whose forward rows are stored (ok: the lane's member can
// still be valid; nothing of any other lane is written).  gp: the pair's table [K][NS], zero on entry;
// gam: the pair's block [T][Smax] or NULL.  Returns whether every D_t, t < n, was > 0 with a finite 1 / D_t.
template <int NS>
__device__ __forceinline__ bool dfb_backward(const unsigned char *tab, const double2 *tr, int j0, int K, int Smax,
                                             const int32_t *__restrict__ sr, int n, int nmax, const double *rows, bool ok,
                                             double *__restrict__ gp, double *__restrict__ gam)
{
    double bh[NS];
#pragma unroll
    for (int j = 0; j < NS; j++) bh[j] = 0.0;
    bool valid = ok;
    int k = sr[nmax - 1], kup = k;  // row t's symbol and row t + 1's
    for (int t = nmax - 1; t >= 0; t--) {
        const int kdn = sr[max(t - 1, 0)];  // the row below, asked for before this row's cells
        double a[NS];
#pragma unroll
        for (int j = 0; j < NS; j++) a[j] = j >= j0 ? rows[((size_t)t * NS + j) * 64] : 0.0;
        // w_t from Bh_{t+1}: all zeros while t >= n - 1 (a zero row stays zero), so Bh_{n-1} is set below
        const double2 *erow = (const double2 *)(tab + (unsigned)min((unsigned)kup, (unsigned)(K - 1)) * dhmm_pitch(NS));
#pragma unroll
        for (int i = 0; i < NS / 2; i++) {
            const double2 e = erow[i];
            bh[2 * i] = e.x * bh[2 * i];
            bh[2 * i + 1] = e.y * bh[2 * i + 1];
        }
        // slots in ascending order: slot j reads the products of slots j and j+1 only; d[s] sits with slot j+1
#pragma unroll
        for (int j = 0; j < NS; j++) {
            const double st = tr[j].x;
            if (j + 1 < NS)
                bh[j] = st * bh[j] + tr[j + 1].y * bh[j + 1];
            else
                bh[j] = st * bh[j];
        }
        dfb_rescale<NS>(bh);
        if (t == n - 1) bh[NS - 1] = 1.0;
        double D = 0.0;
#pragma unroll
        for (int j = 0; j < NS; j++) {
            a[j] = a[j] * bh[j];
            D = j == 0 ? a[0] : D + a[j];
        }
        const double r = 1.0 / D;
        const bool live = ok && t < n, fine = D > 0.0 && r < (double)INFINITY;
        if (live && !fine) valid = false;
        if (live && fine) {
            double *__restrict__ g = gp + (size_t)min((unsigned)k, (unsigned)(K - 1)) * NS;
#pragma unroll
            for (int j = 0; j < NS; j++) {
                if (j < j0) continue;
                const double gm = a[j] * r;
                g[j] = g[j] + gm;
                if (gam) gam[(size_t)t * Smax + (j - j0)] = gm;
            }
        }
        kup = k;
        k = kdn;
    }
    return valid;
}
#pragma clang fp contract(on)

// Every model c = 0 .. nc-1 of this launch (rec and n_states already point at the first one, model c0 of the
// set) against all N sequences: the result of (sequence r, model c) at [r * C + c0 + c].  Dynamic LDS:
// dhmm_lds_bytes(K, NS).
template <int NS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, NS == 32 ? 2 : 8))) void dhmm_fwd(
    const double *__restrict__ rec, const int32_t *__restrict__ n_states, int c0, int nc, int64_t C, int Smax, int K,
    const int32_t *__restrict__ sym, const int32_t *__restrict__ len, int64_t N, int T, double *__restrict__ mant,
    int32_t *__restrict__ expo)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dfb_lds[];
    const int lane = (int)threadIdx.x;
    const double2 *tr = (const double2 *)(dfb_lds + dhmm_tr_offset(K, NS));
    int staged = -1;
    csr_walk((int)gridDim.x, (int)blockIdx.x, nc, nullptr, 0, (int)N, nullptr, len, N, T, [&](int cg, const CsrLane &ln) {
        const int S = n_states[cg];
        double m = 0.0;
        int e = 0;
        if (S >= 1 && S <= Smax && ln.lmax > 0) {
            if (staged != cg) {
                dhmm_stage<NS>(dfb_lds, rec + (size_t)cg * dhmm_record(K, NS), K, lane);
                staged = cg;
            }
            dfb_forward<NS, false>(dfb_lds, tr, NS - S, K, sym + (int64_t)ln.row * T, ln.len, ln.lmax, nullptr, m, e);
        }
        if (!ln.inr) return;
        const int64_t at = ln.p * C + c0 + cg;
        if (mant) mant[at] = m;
        if (expo) expo[at] = e;
    });
}

// The CSR pairs of the window [p_lo, p_hi) under the models of this launch (group_start points at the first
// one's entry): mant, expo, gamma indexed by the pair p, gp by p - p_lo, pvalid[p] = 1 for a valid member.
// rows_ws: T * NS * 64 doubles per wave.
template <int NS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, NS == 32 ? 2 : 8))) void dhmm_fb(
    const double *__restrict__ rec, const int32_t *__restrict__ n_states, int nc, int Smax, int K,
    const int32_t *__restrict__ sym, const int32_t *__restrict__ len, int64_t N, int T,
    const int32_t *__restrict__ group_start, const int32_t *__restrict__ members, int p_lo, int p_hi,
    double *__restrict__ mant, int32_t *__restrict__ expo, double *__restrict__ gamma, double *__restrict__ gp,
    int32_t *__restrict__ pvalid, double *rows_ws)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dfb_lds[];
    const int lane = (int)threadIdx.x, wv = (int)blockIdx.x;
    const double2 *tr = (const double2 *)(dfb_lds + dhmm_tr_offset(K, NS));
    double *rows = rows_ws + (size_t)wv * (size_t)T * NS * 64 + lane;
    int staged = -1;
    csr_walk((int)gridDim.x, wv, nc, group_start, p_lo, p_hi, members, len, N, T, [&](int cg, const CsrLane &ln) {
        const int S = n_states[cg], n = ln.len;
        const int64_t p = ln.p;
        double m = 0.0;
        int e = 0;
        bool valid = false;
        if (S >= 1 && S <= Smax && ln.lmax > 0) {
            if (staged != cg) {
                dhmm_stage<NS>(dfb_lds, rec + (size_t)cg * dhmm_record(K, NS), K, lane);
                staged = cg;
            }
            const int32_t *__restrict__ sr = sym + (int64_t)ln.row * T;
            dfb_forward<NS, true>(dfb_lds, tr, NS - S, K, sr, n, ln.lmax, rows, m, e);
            const bool ok = ln.inr && m > 0.0;  // D_{n-1} is the forward result
            double *__restrict__ gam = gamma && ok ? gamma + (size_t)p * T * Smax : nullptr;
            valid = dfb_backward<NS>(dfb_lds, tr, NS - S, K, Smax, sr, n, ln.lmax, rows, ok,
                                     gp + (ok ? (size_t)(p - p_lo) * K * NS : 0), gam);
            if (gam && !valid)  // a member that turned out invalid: its block back to zeros
                for (int i = 0; i < n * Smax; i++) gam[i] = 0.0;
        }
        if (!ln.inr) return;
        if (mant) mant[p] = m;
        if (expo) expo[p] = e;
        pvalid[p] = valid ? 1 : 0;
    });
}

#pragma clang fp contract(off)
// A thread per (model, symbol, slot): occ_emit[c, s, k] += the G_p of the window's valid members of model c
// in list order; the thread of (symbol 0, last slot) adds their number to n_valid[c].
__global__ __launch_bounds__(256) void dhmm_fb_sum(const int32_t *__restrict__ n_states, int64_t C, int Smax, int K, int NS,
                                                   const int32_t *__restrict__ group_start, int p_lo, int p_hi,
                                                   const int32_t *__restrict__ pvalid, const double *__restrict__ gp,
                                                   double *__restrict__ occ_emit, int32_t *__restrict__ n_valid)
{
    const int64_t R = (int64_t)K * NS, total = C * R;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t c = e / R;
        const int r = (int)(e % R), k = r / NS, j = r % NS;
        const int S = n_states[c], s = j - (NS - S);
        if (S < 1 || S > Smax || s < 0) continue;
        const int g0 = clampi(group_start[c], p_lo, p_hi), g1 = clampi(group_start[c + 1], p_lo, p_hi);
        if (g1 <= g0) continue;
        double *__restrict__ out = occ_emit + ((size_t)c * Smax + s) * K + k;
        double acc = *out;
        int nv = 0;
        for (int p0 = g0; p0 < g1; p0 += HMM_BATCH) {
            bool ok[HMM_BATCH];
            double g[HMM_BATCH];
#pragma unroll
            for (int u = 0; u < HMM_BATCH; u++) {
                const bool in_group = p0 + u < g1;
                ok[u] = in_group && pvalid[p0 + u] != 0;
                g[u] = in_group ? gp[(size_t)(p0 + u - p_lo) * R + r] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < HMM_BATCH; u++) {
                if (!ok[u]) continue;
                acc = acc + g[u];
                nv++;
            }
        }
        *out = acc;
        if (k == 0 && j == NS - 1) n_valid[c] += nv;
    }
}
#pragma clang fp contract(on)

// label [N]: the column of the largest mant * 2^expo per row, zero likelihoods (mant == 0) left out; the
// larger expo, then the larger mant, ties to the smaller index; -1 when every likelihood is zero
__global__ __launch_bounds__(256) void dhmm_fb_label(const double *__restrict__ mant, const int32_t *__restrict__ expo,
                                                     int64_t N, int64_t C, int32_t *__restrict__ label)
{
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < N; r += (int64_t)gridDim.x * 256) {
        double bm = 0.0;
        int32_t be = 0, arg = -1;
        for (int64_t c = 0; c < C; c++) {
            const double m = mant[r * C + c];
            const int32_t e = expo[r * C + c];
            if (m > 0.0 && (arg < 0 || e > be || (e == be && m > bm))) {
                bm = m;
                be = e;
                arg = (int32_t)c;
            }
        }
        label[r] = arg;
    }
}

// ---- host side ----
// workspace: [records of the C models][A rows of G waves][G_p tables of a chunk of PC pairs][a flag per
// pair][mant [N, C] and expo [N, C], for labels without them]
struct DfbPlan {
    int NS, G;
    int64_t PC;
    size_t rec, rows, gp, pvalid, mant, expo;
    size_t total() const { return rec + rows + gp + pvalid + mant + expo; }
};
// bytes of A rows a persistent wave owns in the workspace: [row][slot][lane] doubles
static size_t dfb_rows_bytes(int T, int NS) { return (size_t)T * NS * 512; }
static DfbPlan dfb_plan(int64_t C, int64_t N, int64_t P, int T, int Smax, int K)
{
    DfbPlan pl;
    pl.NS = dhmm_slots(Smax);
    pl.G = csr_waves(P / 64 + std::min<int64_t>(C, HMM_GCHUNK), dfb_rows_bytes(T, pl.NS));
    pl.PC = std::min<int64_t>(P, std::max<int64_t>(64, (int64_t)(DHMM_GP_CAP / ((size_t)K * pl.NS * 8))));
    pl.rec = up256((size_t)C * dhmm_record(K, pl.NS) * 8 + 8);  // never 0, which says "outside the plan"
    pl.rows = P > 0 ? up256(pl.G * dfb_rows_bytes(T, pl.NS)) : 0;
    pl.gp = up256((size_t)pl.PC * K * pl.NS * 8);
    pl.pvalid = up256((size_t)P * 4);
    pl.mant = up256((size_t)N * C * 8);
    pl.expo = up256((size_t)N * C * 4);
    return pl;
}

}  // namespace dsp

extern "C" size_t dsp_dhmm_fb_workspace_bytes(int64_t C, int64_t N, int64_t P, int T, int Smax, int K)
{
    if (!dsp::dhmm_in_plan(C, N, P, T, Smax, K)) return 0;
    return dsp::dfb_plan(C, N, P, T, Smax, K).total();
}

extern "C" int dsp_dhmm_forward(const double *pemit, const double *pstay, const double *padv, const int32_t *n_states,
                                int64_t C, int Smax, int K, const int32_t *sym, const int32_t *len, int64_t N, int T,
                                double *mant, int32_t *expo, int32_t *label, void *workspace, size_t workspace_bytes,
                                void *stream)
{
    using namespace dsp;
    if (!dhmm_in_plan(C, N, 0, T, Smax, K)) return DSP_ERR_ARGS;
    if (N == 0 || (!mant && !expo && !label)) return DSP_OK;
    if (!sym || !len || (C > 0 && (!pemit || !pstay || !padv || !n_states))) return DSP_ERR_ARGS;
    const DfbPlan pl = dfb_plan(C, N, 0, T, Smax, K);
    if (!workspace || workspace_bytes < pl.total()) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    if (label && !mant) mant = (double *)(ws + pl.rec + pl.rows + pl.gp + pl.pvalid);
    if (label && !expo) expo = (int32_t *)(ws + pl.rec + pl.rows + pl.gp + pl.pvalid + pl.mant);
    if (C > 0) {
        double *rec = (double *)ws;
        const int NS = pl.NS;
        const size_t R = dhmm_record(K, NS), lds = dhmm_lds_bytes(K, NS);
        hipLaunchKernelGGL(dhmm_pack, csr_grid(C * (int64_t)R), dim3(256), 0, s, pemit, pstay, padv, n_states, C, Smax, K,
                           NS, rec);
        for (int64_t c0 = 0; c0 < C; c0 += HMM_GCHUNK) {
            const int64_t nc = std::min<int64_t>(HMM_GCHUNK, C - c0);
            const dim3 grid((unsigned)csr_waves(nc * ((N + 63) / 64), 0));
            const double *rc = rec + (size_t)c0 * R;
            const hipError_t e = dhmm_with_slots(NS, [&](auto ns) {
                constexpr int SLOTS = decltype(ns)::value;
                const hipError_t err = dhmm_lds_limit(dhmm_fwd<SLOTS>, lds);
                if (err == hipSuccess)
                    hipLaunchKernelGGL(dhmm_fwd<SLOTS>, grid, dim3(64), lds, s, rc, n_states + c0, (int)c0, (int)nc, C, Smax, K, sym,
                                       len, N, T, mant, expo);
                return err;
            });
            if (e != hipSuccess) return DSP_ERR_HIP + (int)e;
        }
    }
    if (label) hipLaunchKernelGGL(dhmm_fb_label, csr_grid(N), dim3(256), 0, s, mant, expo, N, C, label);
    return dtw_launch_status();
}

extern "C" int dsp_dhmm_expect(const double *pemit, const double *pstay, const double *padv, const int32_t *n_states,
                               int64_t C, int Smax, int K, const int32_t *sym, const int32_t *len, int64_t N, int T,
                               const int32_t *group_start, const int32_t *members, int64_t P, double *mant, int32_t *expo,
                               double *gamma, double *occ_emit, int32_t *n_valid, void *workspace, size_t workspace_bytes,
                               void *stream)
{
    using namespace dsp;
    if (!dhmm_in_plan(C, N, P, T, Smax, K)) return DSP_ERR_ARGS;
    if (C == 0) return DSP_OK;
    if (!pemit || !pstay || !padv || !n_states || !group_start || !occ_emit || !n_valid || (P > 0 && !members) ||
        (N > 0 && (!sym || !len)))
        return DSP_ERR_ARGS;
    const DfbPlan pl = dfb_plan(C, N, P, T, Smax, K);
    if (!workspace || workspace_bytes < pl.total()) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    double *rec = (double *)ws, *rows = (double *)(ws + pl.rec), *gp = (double *)(ws + pl.rec + pl.rows);
    int32_t *pvalid = (int32_t *)(ws + pl.rec + pl.rows + pl.gp);
    const int NS = pl.NS;
    const size_t R = dhmm_record(K, NS), lds = dhmm_lds_bytes(K, NS);
    const dim3 block(256);
    hipLaunchKernelGGL((csr_zero<double, int32_t>), csr_grid(C * Smax * (int64_t)K + C), block, 0, s, occ_emit,
                       C * Smax * (int64_t)K, n_valid, C);
    if (P == 0) return dtw_launch_status();
    if (gamma)
        hipLaunchKernelGGL((csr_zero<double, int32_t>), csr_grid(P * T * Smax), block, 0, s, gamma, P * T * Smax, nullptr, 0);
    hipLaunchKernelGGL(dhmm_pack, csr_grid(C * (int64_t)R), block, 0, s, pemit, pstay, padv, n_states, C, Smax, K, NS, rec);
    for (int64_t p_lo = 0; p_lo < P; p_lo += pl.PC) {
        const int64_t p_hi = std::min<int64_t>(P, p_lo + pl.PC);
        const int64_t cells = (p_hi - p_lo) * K * NS;
        hipLaunchKernelGGL((csr_zero<double, int32_t>), csr_grid(cells), block, 0, s, gp, cells, nullptr, 0);
        for (int64_t c0 = 0; c0 < C; c0 += HMM_GCHUNK) {
            const int64_t nc = std::min<int64_t>(HMM_GCHUNK, C - c0);
            const dim3 grid((unsigned)std::min(pl.G, csr_waves((p_hi - p_lo) / 64 + nc, dfb_rows_bytes(T, NS))));
            const double *rc = rec + (size_t)c0 * R;
            const hipError_t e = dhmm_with_slots(NS, [&](auto ns) {
                constexpr int SLOTS = decltype(ns)::value;
                const hipError_t err = dhmm_lds_limit(dhmm_fb<SLOTS>, lds);
                if (err == hipSuccess)
                    hipLaunchKernelGGL(dhmm_fb<SLOTS>, grid, dim3(64), lds, s, rc, n_states + c0, (int)nc, Smax, K, sym, len, N, T,
                                       group_start + c0, members, (int)p_lo, (int)p_hi, mant, expo, gamma, gp, pvalid, rows);
                return err;
            });
            if (e != hipSuccess) return DSP_ERR_HIP + (int)e;
        }
        hipLaunchKernelGGL(dhmm_fb_sum, csr_grid(C * (int64_t)K * NS), block, 0, s, n_states, C, Smax, K, NS, group_start,
                           (int)p_lo, (int)p_hi, pvalid, gp, occ_emit, n_valid);
    }
    return dtw_launch_status();
}
