// gnb.hip -- GaussianNB.fit and .predict on gfx950 (include/dsp_audiorec.h: dsp_gnb_fit,
// dsp_gnb_predict), the reference's TraditionalClassifier('naive_bayes') (src/models.py:37-39,
// :52-58): no priors, no sample weights.
//
// Fit.  scikit-learn takes np.mean and np.var (axis 0) of each class's rows and np.var of all
// rows; numpy adds along axis 0 sequentially in row order (D >= 2), so every (class, column) pair
// and every (all rows, column) pair is one dependent chain of fp64 adds -- (C + 1) D independent
// chains.  gnb_fit_kernel keeps them fed the way zscore_fit_kernel (zscore.hip) does: two waves stage
// tiles of rows and labels in LDS while the lanes of the other two own one (class, column) pair
// each and add the tile in row order, the add predicated on the label.  No reordering, no atomics:
// theta, var, epsilon are numpy's bits.  gnb_fit_finish takes the largest all-rows variance and
// adds epsilon to var.
//
// Predict.  jll[c] = log_prior[c] + (nconst[c] - 0.5 Q_c), Q_c = sum_d (x_d - theta_cd)^2 / var_cd
// (GaussianNB._joint_log_likelihood); a lane owns a query, theta and var tiles sit in LDS and are
// read as broadcasts, Q is summed in column order.  Each term of Q is the same correctly rounded
// sub, mul and div as numpy's, so the device's and scikit-learn's jll differ only by the summation
// order of D non-negative terms (numpy sums a row pairwise) and the two trailing operations:
//   |jll_device - jll_sklearn| <= bound_c = 2 (D + 8) 2^-53 (|log_prior_c| + |nconst_c| + Q_c / 2)
// (DESIGN.md §4.7).  A row is certified when the winner's margin over every other class exceeds
// GNB_SAFETY (bound_winner + bound_c) and every score is finite; the caller answers the others
// with scikit-learn itself.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsp_audiorec.h"

// every result below is claimed bit-exact against numpy: no fused multiply-add
#pragma clang fp contract(off)

namespace dsp {

// ---- fit ------------------------------------------------------------------------------------
static constexpr int GF_T = 256;     // threads: GF_CONS consumers, the rest load
static constexpr int GF_CONS = 128;  // consumer lanes: GF_S class slots x GF_C columns
static constexpr int GF_R = 128;     // rows per LDS tile
static constexpr int GF_C = 16;      // columns per workgroup
static constexpr int GF_S = GF_CONS / GF_C;  // class slots per workgroup; slot C is "all rows"

// One tile of one chain: rows [0, rows) of column cp (stride GF_C) with their labels lp, added in
// row order.  PASS 0 adds x and counts the chain's rows, PASS 1 adds (x - m)^2.  acc + -0.0 is acc for
// every acc (also for acc = +-0.0), so the addend of a row of another class is -0.0: the select is on
// the addend, off the chain.  `any` (the all-rows slot) takes every row.
template <int PASS>
__device__ __forceinline__ void gnb_fit_tile(const double *cp, const int32_t *lp, int rows, int slot, bool any,
                                             double m, double &acc, int &n)
{
    auto addend = [&](double v, int32_t label) {
        const bool mine = any | (label == slot);
        if (PASS == 0) {
            n += mine ? 1 : 0;
            return mine ? v : -0.0;
        }
        const double x = v - m;
        const double xx = x * x;
        return mine ? xx : -0.0;
    };
    int r = 0;
    // batches of 8 rows: the LDS reads, then the adds (each waits only for its own read)
    for (; r + 8 <= rows; r += 8) {
        double v[8];
        const int4 l0 = *(const int4 *)(lp + r), l1 = *(const int4 *)(lp + r + 4);
        const int32_t lb[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = cp[(r + u) * GF_C];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = addend(v[u], lb[u]);
#pragma unroll
        for (int u = 0; u < 8; u++) acc = acc + v[u];
    }
    for (; r < rows; r++) acc = acc + addend(cp[r * GF_C], lp[r]);
}

__global__ __launch_bounds__(GF_T) void gnb_fit_kernel(const double *X, const int32_t *y, int64_t N, int D, int C,
                                                       double *theta, double *var, int64_t *class_count,
                                                       double *var_all)
{
    __shared__ double tile[2][GF_R * GF_C];
    __shared__ __attribute__((aligned(16))) int32_t lab[2][GF_R];
    const int tid = threadIdx.x;
    const int c0 = (int)blockIdx.x * GF_C, nc = min(GF_C, D - c0);
    const int col = tid % GF_C, slot = (int)blockIdx.y * GF_S + (tid % GF_CONS) / GF_C;
    const bool consumer = tid < GF_CONS, owns = consumer && col < nc && slot <= C;
    const int64_t ntile = (N + GF_R - 1) / GF_R;
    // loaders: rows [t GF_R, +GF_R) x columns [c0, c0 + nc) and the rows' labels.  Lane l loads
    // column l % GF_C of rows l / GF_C + u NL / GF_C (no division by nc; a row's nc values are
    // contiguous), every load of the tile issued before the first LDS store
    constexpr int NL = GF_T - GF_CONS, RPS = NL / GF_C, LPT = GF_R / RPS;
    static_assert(NL == GF_R, "one label per loader lane");
    auto load = [&](int64_t t, int buf) {
        const int l = tid - GF_CONS, c = l % GF_C, r0 = l / GF_C;
        const int64_t row0 = t * GF_R;
        // rows past N and columns past nc are clamped into the matrix, not predicated: nobody reads
        // them from the tile
        const double *src = X + c0 + (c < nc ? c : nc - 1);
        double v[LPT];
#pragma unroll
        for (int u = 0; u < LPT; u++) {
            const int64_t row = row0 + r0 + u * RPS;
            v[u] = src[(row < N ? row : N - 1) * D];
        }
        const int32_t lv = y[row0 + l < N ? row0 + l : N - 1];
#pragma unroll
        for (int u = 0; u < LPT; u++) tile[buf][(r0 + u * RPS) * GF_C + c] = v[u];
        lab[buf][l] = lv;
    };
    // the chain starts from +0.0, np.add.reduce's own start (it adds the rows to its identity: a class whose
    // rows are all -0.0 in a column has the mean +0.0, every other sum is the same from +0.0 and from -0.0)
    double m = 0.0, acc = 0.0;
    int64_t cnt = 0;
    const bool all = slot == C;
    for (int pass = 0; pass < 2; pass++) {
        acc = 0.0;
        if (!consumer) load(0, 0);
        __syncthreads();
        for (int64_t t = 0; t < ntile; t++) {
            const int buf = (int)(t & 1);
            if (!consumer) {
                if (t + 1 < ntile) load(t + 1, buf ^ 1);
            } else if (owns) {
                const int rows = (int)min((int64_t)GF_R, N - t * GF_R);
                int n = 0;
                if (pass == 0) gnb_fit_tile<0>(tile[buf] + col, lab[buf], rows, slot, all, m, acc, n);
                else gnb_fit_tile<1>(tile[buf] + col, lab[buf], rows, slot, all, m, acc, n);
                cnt += n;
            }
            __syncthreads();
        }
        if (pass == 0) m = acc / (double)cnt;
    }
    if (owns) {
        const double v = acc / (double)cnt;
        if (all) {
            var_all[c0 + col] = v;
        } else {
            theta[(int64_t)slot * D + c0 + col] = m;
            var[(int64_t)slot * D + c0 + col] = v;  // epsilon is added by gnb_fit_finish
            if (blockIdx.x == 0 && col == 0) class_count[slot] = cnt;
        }
    }
}

// epsilon = var_smoothing * max_c var_all[c] (np.var(X, axis=0).max(): a NaN wins), var += epsilon
__global__ __launch_bounds__(256) void gnb_fit_finish(const double *var_all, int D, int C, double var_smoothing,
                                                      double *var, double *epsilon)
{
    __shared__ double red[256];
    __shared__ int bad[256];
    const int tid = threadIdx.x;
    double mx = -INFINITY;
    int nan = 0;
    for (int c = tid; c < D; c += 256) {
        const double v = var_all[c];
        nan |= v != v;
        mx = v > mx ? v : mx;
    }
    red[tid] = mx;
    bad[tid] = nan;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            red[tid] = red[tid + w] > red[tid] ? red[tid + w] : red[tid];
            bad[tid] |= bad[tid + w];
        }
        __syncthreads();
    }
    const double eps = var_smoothing * (bad[0] ? (double)NAN : red[0]);
    if (blockIdx.x == 0 && tid == 0) epsilon[0] = eps;
    const int64_t e = (int64_t)blockIdx.x * 256 + tid;
    if (e < (int64_t)C * D) var[e] = var[e] + eps;
}

// ---- predict --------------------------------------------------------------------------------
static constexpr int GNB_T = 128;       // queries per workgroup (one per lane)
static constexpr int GNB_STAGE = 2048;  // theta / var values per LDS stage
static constexpr double GNB_SAFETY = 4.0;

struct GnbArgs {
    const double *theta, *var, *log_prior, *nconst, *X;
    int64_t Nq;
    int D, C;
    double *jll;    // [Nq, C]: the caller's, or scratch
    double *halfq;  // [Nq, C] scratch: Q / 2 for the bound
    int32_t *pred, *certified, *uncertified;
};

// DP = 16 / 32: D <= DP, the query in registers (columns D.. hold theta 0, var 1 and x 0: they
// add +0.0 to a sum that is never -0.0).  DP = 0: any D, the query read from memory.
template <int DP>
__global__ __launch_bounds__(GNB_T) void gnb_predict_kernel(const GnbArgs a)
{
    constexpr bool REG = DP != 0;
    __shared__ double s_t[GNB_STAGE], s_v[GNB_STAGE];
    const int tid = threadIdx.x;
    const int64_t q_raw = (int64_t)blockIdx.x * GNB_T + tid;
    const bool live = q_raw < a.Nq;
    const int64_t qi = live ? q_raw : a.Nq - 1;  // idle lanes shadow the last query (barriers are block-wide)
    const int C = a.C, D = a.D;
    const double *qrow = a.X + qi * D;
    double *jrow = a.jll + qi * C, *hrow = a.halfq + qi * C;

    double q[REG ? DP : 1];
    if constexpr (REG) {
#pragma unroll
        for (int d = 0; d < DP; d++) q[d] = d < D ? qrow[d] : 0.0;
    }
    // a stage holds G whole classes (D <= GNB_STAGE / 2 ...) or one chunk of one class
    const int chunk = REG ? DP : (D < GNB_STAGE ? D : GNB_STAGE);
    const int G = GNB_STAGE / chunk;
    double Q = 0.0;
    for (int c0 = 0; c0 < C; c0 += G) {
        const int ncl = C - c0 < G ? C - c0 : G;
        for (int d0 = 0; d0 < D; d0 += chunk) {
            const int nd = D - d0 < chunk ? D - d0 : chunk;
            __syncthreads();  // the previous stage is consumed
            for (int e = tid; e < ncl * chunk; e += GNB_T) {
                const int j = e / chunk, i = e - j * chunk;
                const bool in = i < nd;
                const int64_t g = (int64_t)(c0 + j) * D + d0 + i;
                s_t[e] = in ? a.theta[g] : 0.0;
                s_v[e] = in ? a.var[g] : 1.0;
            }
            __syncthreads();
            for (int j = 0; j < ncl; j++) {
                const double *t = s_t + j * chunk, *v = s_v + j * chunk;
                if (d0 == 0) Q = 0.0;
                if constexpr (REG) {
#pragma unroll
                    for (int d = 0; d < DP; d++) {
                        const double diff = q[d] - t[d];
                        Q = Q + (diff * diff) / v[d];
                    }
                } else {
                    for (int i = 0; i < nd; i++) {
                        const double diff = qrow[d0 + i] - t[i];
                        Q = Q + (diff * diff) / v[i];
                    }
                }
                if (d0 + nd == D && live) {
                    const int c = c0 + j;
                    const double h = 0.5 * Q;
                    jrow[c] = a.log_prior[c] + (a.nconst[c] - h);
                    hrow[c] = h;
                }
            }
        }
    }
    if (!live) return;
    // the lane reads back what it wrote: the first index of the largest score, then the certificate
    int best = 0;
    double jb = jrow[0];
    bool finite = true;
    for (int c = 0; c < C; c++) {
        const double j = jrow[c];
        finite = finite && (fabs(j) < INFINITY);  // (false for a NaN)
        if (j > jb) {
            jb = j;
            best = c;
        }
    }
    const double k = 2.0 * (double)(D + 8) * 0x1p-53;
    const double bb = k * (fabs(a.log_prior[best]) + fabs(a.nconst[best]) + hrow[best]);
    bool cert = finite;
    for (int c = 0; c < C; c++) {
        if (c == best) continue;
        const double bc = k * (fabs(a.log_prior[c]) + fabs(a.nconst[c]) + hrow[c]);
        cert = cert && (jb - jrow[c] > GNB_SAFETY * (bb + bc));
    }
    a.pred[q_raw] = best;
    a.certified[q_raw] = cert ? 1 : 0;
    if (!cert) atomicAdd(a.uncertified, 1);
}

// the uncertified count starts at 0 by a kernel's store, not a memset node (as svc_prep's, svm.hip):
// a captured call is a plain chain of kernels.  gnb_predict_kernel has no kernel before it and its
// workgroups are not ordered among themselves, so the store is a launch of its own
__global__ void gnb_clear(int32_t *uncertified) { uncertified[0] = 0; }

}  // namespace dsp

namespace {
static constexpr int GNB_DMAX = 4096, GNB_CMAX = 64;
static constexpr size_t GNB_HEAD = 256;  // the counter's slot at the start of the workspace

size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

bool gnb_args_ok(int64_t Nq, int D, int C)
{
    return Nq >= 0 && D >= 1 && D <= GNB_DMAX && C >= 1 && C <= GNB_CMAX;
}
}  // namespace

extern "C" int dsp_gnb_fit(const double *X, const int32_t *y, int64_t N, int D, int C, double var_smoothing,
                           double *theta, double *var, int64_t *class_count, double *epsilon, void *workspace,
                           size_t workspace_bytes, void *stream)
{
    if (N < 1 || D < 2 || D > GNB_DMAX || C < 1 || C > GNB_CMAX || !X || !y || !theta || !var || !class_count ||
        !epsilon)
        return DSP_ERR_ARGS;
    if (!workspace || workspace_bytes < (size_t)D * 8) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double *var_all = (double *)workspace;
    const dim3 grid((unsigned)((D + dsp::GF_C - 1) / dsp::GF_C), (unsigned)((C + 1 + dsp::GF_S - 1) / dsp::GF_S));
    hipLaunchKernelGGL(dsp::gnb_fit_kernel, grid, dim3(dsp::GF_T), 0, s, X, y, N, D, C, theta, var, class_count,
                       var_all);
    hipLaunchKernelGGL(dsp::gnb_fit_finish, dim3((unsigned)(((int64_t)C * D + 255) / 256)), dim3(256), 0, s, var_all,
                       D, C, var_smoothing, var, epsilon);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
}

extern "C" size_t dsp_gnb_workspace_bytes(int64_t Nq, int D, int C)
{
    if (!gnb_args_ok(Nq, D, C)) return 0;
    return GNB_HEAD + 2 * al((size_t)Nq * C * 8);
}

extern "C" int dsp_gnb_predict(const double *theta, const double *var, const double *log_prior, const double *nconst,
                               int D, int C, const double *X, int64_t Nq, int32_t *pred, double *jll,
                               int32_t *certified, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!gnb_args_ok(Nq, D, C) || !theta || !var || !log_prior || !nconst) return DSP_ERR_ARGS;
    if (Nq > 0 && (!X || !pred || !certified)) return DSP_ERR_ARGS;
    if (!workspace || workspace_bytes < dsp_gnb_workspace_bytes(Nq, D, C)) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const int64_t blocks = (Nq + dsp::GNB_T - 1) / dsp::GNB_T;
    if (blocks > 0x7fffffff) return DSP_ERR_ARGS;
    hipLaunchKernelGGL(dsp::gnb_clear, dim3(1), dim3(1), 0, s, (int32_t *)ws);
    if (Nq == 0) return hipGetLastError() == hipSuccess ? DSP_OK : DSP_ERR_HIP;
    dsp::GnbArgs a;
    a.theta = theta, a.var = var, a.log_prior = log_prior, a.nconst = nconst, a.X = X;
    a.Nq = Nq, a.D = D, a.C = C;
    a.halfq = (double *)(ws + GNB_HEAD);
    a.jll = jll ? jll : (double *)(ws + GNB_HEAD + al((size_t)Nq * C * 8));
    a.pred = pred, a.certified = certified, a.uncertified = (int32_t *)ws;
    const dim3 grid((unsigned)blocks), block(dsp::GNB_T);
    if (D <= 16) hipLaunchKernelGGL(dsp::gnb_predict_kernel<16>, grid, block, 0, s, a);
    else if (D <= 32) hipLaunchKernelGGL(dsp::gnb_predict_kernel<32>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(dsp::gnb_predict_kernel<0>, grid, block, 0, s, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
}
