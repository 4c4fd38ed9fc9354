// mlp.hip -- the reference's MLP classifier (src/models.py:77-221) on one CU per model.
//
// dsp_mlp_train: a persistent single-workgroup kernel per model.  Parameters, one batch of
// activations and the logits live in LDS for the whole launch; Adam's moments stay in global
// memory (L2 resident, touched once per step by the thread that owns the gradient element).
// One step = gather the batch, forward (4x4 register tiles, float4 LDS reads), softmax / loss,
// and per layer from the top: dW tile into registers -> delta of the layer below written in
// place over that layer's activations -> Adam on the layer from the registers.  Every sum has a
// fixed order (no atomics), so a launch is reproducible bit for bit.  DESIGN.md §4.5.
//
// dsp_mlp_predict: the same forward tiles over 64 rows per workgroup, no dropout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dsp_audiorec.h"
#include "dsp_device.h"

namespace dsp {
namespace mlp {

constexpr int NT_TRAIN = 512;
constexpr int NT_PRED = 256;
constexpr int PRED_ROWS = 64;
constexpr int MAX_LIN = DSP_MLP_MAX_HIDDEN + 1;  // linear layers
constexpr int MAX_W = 64;                        // widest layer (input included) of the fused plan
constexpr size_t LDS_LIMIT = 160 * 1024;

// LDS carve-up (float offsets, every piece a multiple of 4 floats = 16 B).
struct Plan {
    int nl;                 // linear layers
    int dim[MAX_LIN + 1];   // D, hidden..., C
    int poff[MAX_LIN];      // weight of layer l in the packed (nn.Linear) buffer; bias follows it
    int woff[MAX_LIN];      // W_l in LDS: roundup4(out) rows of wst[l] floats, zero padded
    int wst[MAX_LIN];       // roundup4(in) + 4: rows o, o + 16, ... of one lane on different banks
    int boff[MAX_LIN];      // bias_l in LDS
    int aoff[MAX_LIN + 1];  // act[k]: input of layer k (act[nl] = logits), rows x ast[k]
    int ast[MAX_LIN + 1];   // roundup4(dim[k])
    int rowloss, rowcorr, scal;
    int rows;
    int nparam;
    int total;  // floats
};

__host__ __device__ inline int r4(int x) { return (x + 3) & ~3; }

// returns false when the configuration is outside the fused plan
static bool make_plan(Plan &p, int D, int n_hidden, const int *hidden, int C, int rows, bool train)
{
    if (D < 1 || D > MAX_W || n_hidden < 0 || n_hidden > DSP_MLP_MAX_HIDDEN || C < 1 || C > MAX_W || rows < 1 ||
        rows > 4096 || (n_hidden > 0 && !hidden))
        return false;
    p.nl = n_hidden + 1;
    p.dim[0] = D;
    for (int i = 0; i < n_hidden; i++) {
        if (hidden[i] < 1 || hidden[i] > MAX_W) return false;
        p.dim[i + 1] = hidden[i];
    }
    p.dim[p.nl] = C;
    for (int i = p.nl + 1; i <= MAX_LIN; i++) p.dim[i] = 0;
    int off = 0, np = 0;
    for (int l = 0; l < MAX_LIN; l++) {
        p.poff[l] = p.woff[l] = p.wst[l] = p.boff[l] = 0;
        if (l >= p.nl) continue;
        const int in = p.dim[l], out = p.dim[l + 1];
        p.poff[l] = np;
        np += out * in + out;
        p.wst[l] = r4(in) + 4;
        p.woff[l] = off;
        off += r4(out) * p.wst[l];
        p.boff[l] = off;
        off += r4(out);
    }
    p.nparam = np;
    p.rows = rows;
    for (int k = 0; k <= MAX_LIN; k++) p.aoff[k] = p.ast[k] = 0;
    if (train) {
        for (int k = 0; k <= p.nl; k++) {
            p.ast[k] = r4(p.dim[k]);
            p.aoff[k] = off;
            off += rows * p.ast[k];
        }
    } else {  // act[0], then two buffers the layers alternate between
        int wmax = 0;
        for (int k = 1; k <= p.nl; k++) wmax = r4(p.dim[k]) > wmax ? r4(p.dim[k]) : wmax;
        p.ast[0] = r4(D);
        p.aoff[0] = off;
        off += rows * p.ast[0];
        for (int k = 1; k <= p.nl; k++) {
            p.ast[k] = r4(p.dim[k]);
            p.aoff[k] = off + (k & 1) * rows * wmax;
        }
        off += 2 * rows * wmax;
    }
    p.rowloss = off;
    off += r4(rows);
    p.rowcorr = off;
    off += r4(rows);
    p.scal = off;
    off += 4;
    p.total = off;
    return (size_t)off * sizeof(float) <= LDS_LIMIT;
}

// ---- dropout hash (include/dsp_audiorec.h states the definition the tests restate) -----------
__host__ __device__ inline uint32_t mix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
// the part that is uniform over one layer of one step
__host__ __device__ inline uint32_t drop_layer_key(uint32_t seed, int64_t step, int layer)
{
    uint32_t h = mix32(seed + 0x9e3779b9u);
    h = mix32(h ^ (uint32_t)((uint64_t)step & 0xffffffffu));
    h = mix32(h ^ (uint32_t)((uint64_t)step >> 32));
    return mix32(h ^ (uint32_t)layer);
}
__host__ __device__ inline uint32_t drop_hash(uint32_t layer_key, int row, int unit)
{
    return mix32(mix32(layer_key ^ (uint32_t)row) ^ (uint32_t)unit);
}

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

// act_out[b][o] = f(bias[o] + sum_i act_in[b][i] W[o][i]); a thread owns rows 4bt..4bt+3 and
// outputs ot, ot+16, ..: 16 lanes read 16 different W rows (stride wst: different banks) and
// broadcast the activation rows.  hidden: ReLU, then dropout when thr != 0.
template <int NJ>
__device__ __forceinline__ void forward_tiles(const float *W, int wst, const float *bias, const float *ain, int ast,
                                              float *aout, int ost, int rows, int n_in, int n_out, bool hidden,
                                              uint32_t lkey, uint32_t thr, float scale)
{
    const int nbt = (rows + 3) >> 2, n4 = r4(n_in) >> 2, outp = r4(n_out);
    for (int t = threadIdx.x; t < nbt * 16; t += blockDim.x) {
        const int ot = t & 15, bt = t >> 4;
        float acc[4][NJ];
        const float *ap[4], *wp[NJ];
#pragma unroll
        for (int r = 0; r < 4; r++) ap[r] = ain + min(4 * bt + r, rows - 1) * ast;
#pragma unroll
        for (int j = 0; j < NJ; j++) wp[j] = W + min(ot + 16 * j, outp - 1) * wst;
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int j = 0; j < NJ; j++) acc[r][j] = 0.f;
        for (int k = 0; k < n4; k++) {
            float4 a[4], w[NJ];
#pragma unroll
            for (int r = 0; r < 4; r++) a[r] = ld4(ap[r] + 4 * k);
#pragma unroll
            for (int j = 0; j < NJ; j++) w[j] = ld4(wp[j] + 4 * k);
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int j = 0; j < NJ; j++) {
                    float s = acc[r][j];
                    s = fmaf(a[r].x, w[j].x, s);
                    s = fmaf(a[r].y, w[j].y, s);
                    s = fmaf(a[r].z, w[j].z, s);
                    s = fmaf(a[r].w, w[j].w, s);
                    acc[r][j] = s;
                }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int b = 4 * bt + r;
            if (b >= rows) continue;
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                const int o = ot + 16 * j;
                if (o >= outp) continue;
                float v = 0.f;
                if (o < n_out) {
                    v = acc[r][j] + bias[o];
                    if (hidden) {
                        v = v > 0.f ? v : 0.f;
                        if (thr != 0u) v = drop_hash(lkey, b, o) < thr ? 0.f : v * scale;
                    }
                }
                aout[b * ost + o] = v;
            }
        }
    }
}

__device__ __forceinline__ void forward_layer(const Plan &p, float *lds, int l, int rows, uint32_t lkey, uint32_t thr,
                                              float scale)
{
    const float *W = lds + p.woff[l], *bias = lds + p.boff[l], *ain = lds + p.aoff[l];
    float *aout = lds + p.aoff[l + 1];
    const int n_in = p.dim[l], n_out = p.dim[l + 1];
    const bool hidden = l + 1 < p.nl;
    const int nj = (r4(n_out) + 15) >> 4;  // block-uniform
    if (nj == 1) forward_tiles<1>(W, p.wst[l], bias, ain, p.ast[l], aout, p.ast[l + 1], rows, n_in, n_out, hidden, lkey, thr, scale);
    else if (nj == 2) forward_tiles<2>(W, p.wst[l], bias, ain, p.ast[l], aout, p.ast[l + 1], rows, n_in, n_out, hidden, lkey, thr, scale);
    else if (nj == 3) forward_tiles<3>(W, p.wst[l], bias, ain, p.ast[l], aout, p.ast[l + 1], rows, n_in, n_out, hidden, lkey, thr, scale);
    else forward_tiles<4>(W, p.wst[l], bias, ain, p.ast[l], aout, p.ast[l + 1], rows, n_in, n_out, hidden, lkey, thr, scale);
}

// packed nn.Linear buffer <-> padded LDS copy
__device__ __forceinline__ int lds_index(const Plan &p, int idx)
{
    int l = 0;
#pragma unroll
    for (int q = 1; q < MAX_LIN; q++)
        if (q < p.nl && idx >= p.poff[q]) l = q;
    const int in = p.dim[l], out = p.dim[l + 1], r = idx - p.poff[l];
    if (r < out * in) return p.woff[l] + (r / in) * p.wst[l] + (r % in);
    return p.boff[l] + (r - out * in);
}
__device__ __forceinline__ void load_params(const Plan &p, float *lds, const float *g)
{
    const int nw = p.aoff[0];  // the parameter block comes first
    for (int i = threadIdx.x; i < nw; i += blockDim.x) lds[i] = 0.f;
    __syncthreads();
    for (int i = threadIdx.x; i < p.nparam; i += blockDim.x) lds[lds_index(p, i)] = g[i];
}

__device__ __forceinline__ double ipow(double b, int64_t t)
{
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

// optim.Adam defaults (single-tensor path): m.lerp_(g, 1-b1); v = b2 v + (1-b2) g g;
// denom = sqrt(v) / sqrt(1 - b2^t) + eps; w -= (lr / (1 - b1^t)) * m / denom
__device__ __forceinline__ void adam(float *w, float *m, float *v, float mm, float vv, float g, float step_size,
                                     float bc2s)
{
    mm = mm + (g - mm) * 0.1f;
    vv = vv * 0.999f + (g * g) * 0.001f;
    *m = mm;
    *v = vv;
    const float denom = sqrtf(vv) / bc2s + 1e-8f;
    *w = *w - step_size * (mm / denom);
}

struct TrainArgs {
    const float *X;
    const int32_t *y;
    int64_t N, x_stride, y_stride;
    const int32_t *perm;
    int64_t perm_stride;
    int n_epochs, batch_size;
    float *params, *m, *v;
    int64_t *steps;
    const double *lr;
    const uint32_t *seeds;
    uint32_t thr;
    float scale;
    float *loss_hist, *acc_hist;
    Plan p;
};

__global__ __launch_bounds__(NT_TRAIN) void mlp_train_kernel(const TrainArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Plan &p = a.p;
    const int tid = threadIdx.x, model = blockIdx.x;
    const int D = p.dim[0], C = p.dim[p.nl], nl = p.nl;
    float *gm = a.m + (size_t)model * p.nparam, *gv = a.v + (size_t)model * p.nparam;
    float *gp = a.params + (size_t)model * p.nparam;
    const int32_t *perm = a.perm + (size_t)model * a.perm_stride;
    const float *X = a.X + (size_t)model * a.x_stride;
    const int32_t *y = a.y + (size_t)model * a.y_stride;
    const double lr = a.lr[model];
    const uint32_t seed = a.seeds[model];
    const float scale = a.thr ? a.scale : 1.f;
    int64_t step = a.steps[model];  // optimizer steps done so far
    const int64_t N = a.N;
    const int bsz = a.batch_size;
    const int nb = (int)((N + bsz - 1) / bsz);
    float *rowloss = lds + p.rowloss, *sc = lds + p.scal;
    int *rowcorr = reinterpret_cast<int *>(lds + p.rowcorr);

    load_params(p, lds, gp);
    __syncthreads();

    for (int e = 0; e < a.n_epochs; e++) {
        double eloss = 0.0;  // thread 0: sum of the batches' mean losses, as a Python float
        int ecorr = 0;
        for (int bi = 0; bi < nb; bi++) {
            const int64_t base = (int64_t)bi * bsz;
            const int rows = (int)(N - base < bsz ? N - base : bsz);
            // ---- gather the batch (act[0], zero padded columns) and this step's Adam scalars
            {
                float *a0 = lds + p.aoff[0];
                const int st = p.ast[0];
                for (int i = tid; i < rows * st; i += NT_TRAIN) {
                    const int b = i / st, c = i - b * st;
                    int64_t r = perm[(int64_t)e * N + base + b];
                    r = r < 0 ? 0 : (r >= N ? N - 1 : r);  // a bad index must not leave X
                    a0[i] = c < D ? X[r * D + c] : 0.f;
                    if (c == 0) rowcorr[b] = y[r];  // the row's label, replaced by its hit flag below
                }
                if (tid == 0) {
                    const double bc1 = 1.0 - ipow(0.9, step + 1), bc2 = 1.0 - ipow(0.999, step + 1);
                    sc[0] = (float)(lr / bc1);
                    sc[1] = (float)sqrt(bc2);
                }
            }
            __syncthreads();
            // ---- forward
            for (int l = 0; l < nl; l++) {
                forward_layer(p, lds, l, rows, drop_layer_key(seed, step, l), a.thr, scale);
                __syncthreads();
            }
            // ---- softmax, loss, first-index argmax; logits -> d loss / d logits in place
            {
                float *lg = lds + p.aoff[nl];
                const int st = p.ast[nl];
                const float inv = 1.f / (float)rows;
                for (int b = tid; b < rows; b += NT_TRAIN) {
                    float *z = lg + b * st;
                    int yb = rowcorr[b];
                    yb = yb < 0 ? 0 : (yb >= C ? C - 1 : yb);
                    float mx = z[0];
                    int am = 0;
                    for (int c = 1; c < C; c++)
                        if (z[c] > mx) {
                            mx = z[c];
                            am = c;
                        }
                    float s = 0.f;
                    for (int c = 0; c < C; c++) s += expf(z[c] - mx);
                    const float ls = logf(s);
                    rowloss[b] = ls - (z[yb] - mx);
                    rowcorr[b] = am == yb;
                    for (int c = 0; c < st; c++) {
                        float d = 0.f;
                        if (c < C) d = (expf(z[c] - mx - ls) - (c == yb ? 1.f : 0.f)) * inv;
                        z[c] = d;
                    }
                }
            }
            __syncthreads();
            if (tid < 64) {  // wave 0: batch loss and hits in a fixed order
                float s = 0.f;
                int k = 0;
                for (int b = tid; b < rows; b += 64) {
                    s += rowloss[b];
                    k += rowcorr[b];
                }
                s = wave_sum(s);
                k = wave_sum(k);
                eloss += (double)(s / (float)rows);
                ecorr += k;
            }
            // ---- backward, top layer first
            const float step_size = sc[0], bc2s = sc[1];
            for (int l = nl - 1; l >= 0; l--) {
                const int n_in = p.dim[l], n_out = p.dim[l + 1];
                const int in4 = r4(n_in) >> 2, out4 = r4(n_out) >> 2;
                const float *dl = lds + p.aoff[l + 1];  // delta of this layer's output
                const int dst = p.ast[l + 1];
                float *ai = lds + p.aoff[l];
                const int ist = p.ast[l];
                float *W = lds + p.woff[l];
                const int wst = p.wst[l];
                // A: this thread's 4x4 tile of dW (and db) into registers
                const bool own = tid < out4 * in4;
                const int ot = tid / in4, it = tid - ot * in4;
                float g[4][4], gb[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    gb[k] = 0.f;
#pragma unroll
                    for (int c = 0; c < 4; c++) g[k][c] = 0.f;
                }
                // the tile's Adam moments, loaded now so that their latency hides behind the dW sums
                const int pw = p.poff[l], pb = pw + n_out * n_in;
                float m0[4][4], v0[4][4], mb[4], vb[4];
                if (own) {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int o = 4 * ot + k;
                        const bool ob = o < n_out && it == 0;
                        mb[k] = ob ? gm[pb + o] : 0.f;
                        vb[k] = ob ? gv[pb + o] : 0.f;
#pragma unroll
                        for (int c = 0; c < 4; c++) {
                            const int i = 4 * it + c;
                            const bool in = o < n_out && i < n_in;
                            m0[k][c] = in ? gm[pw + o * n_in + i] : 0.f;
                            v0[k][c] = in ? gv[pw + o * n_in + i] : 0.f;
                        }
                    }
                    const float *dp = dl + 4 * ot, *ap = ai + 4 * it;
#pragma unroll 4
                    for (int b = 0; b < rows; b++) {
                        const float4 d = ld4(dp + b * dst), x = ld4(ap + b * ist);
                        const float dd[4] = {d.x, d.y, d.z, d.w}, xx[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            gb[k] += dd[k];
#pragma unroll
                            for (int c = 0; c < 4; c++) g[k][c] = fmaf(dd[k], xx[c], g[k][c]);
                        }
                    }
                }
                if (l > 0) {
                    __syncthreads();  // every dW tile has read act[l]
                    // B: delta of act[l] in place: (delta W) * (ReLU and dropout derivative)
                    const int nbt = (rows + 3) >> 2;
                    for (int t = tid; t < nbt * in4; t += NT_TRAIN) {
                        const int bt = t / in4, ci = t - bt * in4;
                        float acc[4][4];
#pragma unroll
                        for (int r = 0; r < 4; r++)
#pragma unroll
                            for (int c = 0; c < 4; c++) acc[r][c] = 0.f;
                        const float *dr[4];
#pragma unroll
                        for (int r = 0; r < 4; r++) dr[r] = dl + min(4 * bt + r, rows - 1) * dst;
                        for (int o4 = 0; o4 < out4; o4++) {
                            float4 d[4], w[4];
#pragma unroll
                            for (int r = 0; r < 4; r++) d[r] = ld4(dr[r] + 4 * o4);
#pragma unroll
                            for (int k = 0; k < 4; k++) w[k] = ld4(W + (4 * o4 + k) * wst + 4 * ci);
#pragma unroll
                            for (int r = 0; r < 4; r++) {
                                const float dd[4] = {d[r].x, d[r].y, d[r].z, d[r].w};
#pragma unroll
                                for (int k = 0; k < 4; k++) {
                                    acc[r][0] = fmaf(dd[k], w[k].x, acc[r][0]);
                                    acc[r][1] = fmaf(dd[k], w[k].y, acc[r][1]);
                                    acc[r][2] = fmaf(dd[k], w[k].z, acc[r][2]);
                                    acc[r][3] = fmaf(dd[k], w[k].w, acc[r][3]);
                                }
                            }
                        }
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int b = 4 * bt + r;
                            if (b >= rows) continue;
                            float4 *q = reinterpret_cast<float4 *>(ai + b * ist + 4 * ci);
                            const float4 old = *q;
                            float4 nw;
                            nw.x = old.x > 0.f ? acc[r][0] * scale : 0.f;
                            nw.y = old.y > 0.f ? acc[r][1] * scale : 0.f;
                            nw.z = old.z > 0.f ? acc[r][2] * scale : 0.f;
                            nw.w = old.w > 0.f ? acc[r][3] * scale : 0.f;
                            *q = nw;
                        }
                    }
                    __syncthreads();  // W_l has been read by every delta tile
                }
                // C: Adam on the tile
                if (own) {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int o = 4 * ot + k;
                        if (o >= n_out) continue;
#pragma unroll
                        for (int c = 0; c < 4; c++) {
                            const int i = 4 * it + c;
                            if (i >= n_in) continue;
                            const int gi = pw + o * n_in + i;
                            adam(W + o * wst + i, gm + gi, gv + gi, m0[k][c], v0[k][c], g[k][c], step_size, bc2s);
                        }
                        if (it == 0)
                            adam(lds + p.boff[l] + o, gm + pb + o, gv + pb + o, mb[k], vb[k], gb[k], step_size, bc2s);
                    }
                }
            }
            step++;
            __syncthreads();
        }
        if (tid == 0) {
            a.loss_hist[(size_t)model * a.n_epochs + e] = (float)(eloss / (double)nb);
            a.acc_hist[(size_t)model * a.n_epochs + e] = (float)((double)ecorr / (double)N);
        }
    }
    for (int i = tid; i < p.nparam; i += NT_TRAIN) gp[i] = lds[lds_index(p, i)];
    if (tid == 0) a.steps[model] = step;
}

struct PredArgs {
    const float *params, *X;
    int64_t Nq;
    int32_t *pred;
    float *logits;
    Plan p;
};

__global__ __launch_bounds__(NT_PRED) void mlp_predict_kernel(const PredArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Plan &p = a.p;
    const int tid = threadIdx.x;
    const int D = p.dim[0], C = p.dim[p.nl];
    const int64_t row0 = (int64_t)blockIdx.x * PRED_ROWS;
    const int rows = (int)(a.Nq - row0 < PRED_ROWS ? a.Nq - row0 : PRED_ROWS);
    load_params(p, lds, a.params);
    float *a0 = lds + p.aoff[0];
    const int st = p.ast[0];
    for (int i = tid; i < rows * st; i += NT_PRED) {
        const int b = i / st, c = i - b * st;
        a0[i] = c < D ? a.X[(row0 + b) * D + c] : 0.f;
    }
    __syncthreads();
    for (int l = 0; l < p.nl; l++) {
        forward_layer(p, lds, l, rows, 0u, 0u, 1.f);
        __syncthreads();
    }
    const float *lg = lds + p.aoff[p.nl];
    const int ls = p.ast[p.nl];
    if (tid < rows) {
        const float *z = lg + tid * ls;
        float mx = z[0];
        int am = 0;
        for (int c = 1; c < C; c++)
            if (z[c] > mx) {
                mx = z[c];
                am = c;
            }
        a.pred[row0 + tid] = am;
    }
    if (a.logits)
        for (int i = tid; i < rows * C; i += NT_PRED) {
            const int b = i / C, c = i - b * C;
            a.logits[(row0 + b) * C + c] = lg[b * ls + c];
        }
}

__global__ void mlp_dropout_mask_kernel(uint32_t seed, int64_t step, int layer, int rows, int width, uint32_t thr,
                                        uint8_t *mask)
{
    const uint32_t lkey = drop_layer_key(seed, step, layer);
    const int n = rows * width;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        mask[i] = drop_hash(lkey, i / width, i % width) >= thr;
}

static bool g_attr_done[64];
static int set_lds_attr()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return DSP_ERR_HIP;
    if (!g_attr_done[dev]) {
        (void)hipFuncSetAttribute((const void *)mlp_train_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)LDS_LIMIT);
        (void)hipFuncSetAttribute((const void *)mlp_predict_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)LDS_LIMIT);
        g_attr_done[dev] = true;
    }
    return DSP_OK;
}

}  // namespace mlp
}  // namespace dsp

extern "C" size_t dsp_mlp_lds_bytes(int D, int n_hidden, const int *hidden, int C, int batch_size)
{
    dsp::mlp::Plan p;
    if (!dsp::mlp::make_plan(p, D, n_hidden, hidden, C, batch_size, true)) return 0;
    return (size_t)p.total * sizeof(float);
}

extern "C" int64_t dsp_mlp_param_count(int D, int n_hidden, const int *hidden, int C)
{
    if (D < 1 || C < 1 || n_hidden < 0 || (n_hidden > 0 && !hidden)) return 0;
    int64_t n = 0, prev = D;
    for (int i = 0; i < n_hidden; i++) {
        if (hidden[i] < 1) return 0;
        n += prev * hidden[i] + hidden[i];
        prev = hidden[i];
    }
    return n + prev * C + C;
}

extern "C" int dsp_mlp_train(const float *X, const int32_t *y, int64_t N, int64_t x_stride, int64_t y_stride, int D,
                             int n_hidden, const int *hidden, int C, int n_models, int n_epochs, int batch_size,
                             const int32_t *perm,
                             int64_t perm_stride, float *params, float *m, float *v, int64_t *steps,
                             const double *lr, const uint32_t *seeds, uint32_t drop_threshold, float keep_scale,
                             float *loss_hist, float *acc_hist, void *stream)
{
    using namespace dsp::mlp;
    if (!X || !y || !perm || !params || !m || !v || !steps || !lr || !seeds || !loss_hist || !acc_hist ||
        N < 1 || N > (int64_t)1 << 31 || n_models < 1 || n_epochs < 0 || batch_size < 1 ||
        n_epochs * N > (int64_t)1 << 40 || (perm_stride != 0 && perm_stride < (int64_t)n_epochs * N) ||
        (x_stride != 0 && (D < 1 || x_stride < N * D)) || (y_stride != 0 && y_stride < N))
        return DSP_ERR_ARGS;
    TrainArgs a;
    if (!make_plan(a.p, D, n_hidden, hidden, C, batch_size, true)) return DSP_ERR_ARGS;
    if (n_epochs == 0) return DSP_OK;
    if (set_lds_attr() != DSP_OK) return DSP_ERR_HIP;
    a.X = X;
    a.y = y;
    a.N = N;
    a.x_stride = x_stride;
    a.y_stride = y_stride;
    a.perm = perm;
    a.perm_stride = perm_stride;
    a.n_epochs = n_epochs;
    a.batch_size = batch_size;
    a.params = params;
    a.m = m;
    a.v = v;
    a.steps = steps;
    a.lr = lr;
    a.seeds = seeds;
    a.thr = drop_threshold;
    a.scale = keep_scale;
    a.loss_hist = loss_hist;
    a.acc_hist = acc_hist;
    hipLaunchKernelGGL(mlp_train_kernel, dim3((unsigned)n_models), dim3(NT_TRAIN), (size_t)a.p.total * sizeof(float),
                       (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
}

extern "C" int dsp_mlp_predict(const float *params, const float *X, int64_t Nq, int D, int n_hidden,
                               const int *hidden, int C, int32_t *pred, float *logits, void *stream)
{
    using namespace dsp::mlp;
    if (!params || !X || !pred || Nq < 0 || Nq > ((int64_t)1 << 31) * PRED_ROWS - 1) return DSP_ERR_ARGS;
    PredArgs a;
    if (!make_plan(a.p, D, n_hidden, hidden, C, PRED_ROWS, false)) return DSP_ERR_ARGS;
    if (Nq == 0) return DSP_OK;
    if (set_lds_attr() != DSP_OK) return DSP_ERR_HIP;
    a.params = params;
    a.X = X;
    a.Nq = Nq;
    a.pred = pred;
    a.logits = logits;
    hipLaunchKernelGGL(mlp_predict_kernel, dim3((unsigned)((Nq + PRED_ROWS - 1) / PRED_ROWS)), dim3(NT_PRED),
                       (size_t)a.p.total * sizeof(float), (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
}

extern "C" int dsp_mlp_dropout_mask(uint32_t seed, int64_t step, int layer, int rows, int width,
                                    uint32_t drop_threshold, uint8_t *mask, void *stream)
{
    if (!mask || rows < 1 || width < 1 || layer < 0 || step < 0 || (int64_t)rows * width > (int64_t)1 << 30)
        return DSP_ERR_ARGS;
    const int n = rows * width;
    hipLaunchKernelGGL(dsp::mlp::mlp_dropout_mask_kernel, dim3((unsigned)std::min((n + 255) / 256, 1024)), dim3(256), 0,
                       (hipStream_t)stream, seed, step, layer, rows, width, drop_threshold, mask);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
}
