// lpc.hip -- dsp_lpc_autocorr and dsp_lpc_solve: linear prediction of the crop frames
// (include/dsp_audiorec.h).
//
// The definition.  A clip is x[0..N) int16, its crop [st, en) and frame count nf as
// dsp_extract_features wrote them, L = frame_length, S = frame_shift, p = order.
//   c         = floor((2 sum(x) + N) / (2 N))          the clip mean rounded half up
//   y[n]      = x[n] - c                               |y| <= 65535
//   f_t[i]    = y[st + t S + i] if st + t S + i < en, else 0                0 <= i < L
//   w[i]      = min(max(window[i], 0), 32768)          Q15; window == NULL: z = f
//   z_t[i]    = (f_t[i] w[i] + 16384) >> 15            arithmetic shift; |z| <= |y|
//   r_t(tau)  = sum_{i=0}^{L-1-tau} z_t[i] z_t[i+tau]  tau = 0 .. p, exact int64, |r| < 2^45
// and per row of r, every operation one rounded fp64 operation in this order, never fused:
//   R[j] = (double) r[j];  a[1..p] = k[1..p] = 0;  E = R[0];  m = 0
//   for i = 1..p:
//       if not (E > 0): stop
//       acc = R[i];  for j = 1..i-1 ascending:  acc = acc - a[j] R[i-j]
//       ki = acc / E
//       if not (|ki| < 1): stop
//       for j = 1..i-1:  a'[j] = a[j] - ki a[i-j];   a'[i] = ki;   a = a';   k[i] = ki
//       E = E (1 - ki ki);   m = i
//   err = E;  reached = m
//   for n = 1..Q:
//       s = 0;  for q = max(1, n-p) .. n-1 ascending:  s = s + ((double) q c[q]) a[n-q]
//       c[n] = (n <= p ? a[n] : 0) + s / (double) n
//
// lpc_autocorr: one workgroup of four waves per clip, as pitch.hip.  The workgroup sums the clip (c), then
// each wave takes every fourth frame on its own:
//   stage   z of the frame as int32 in the wave's own LDS image, zeros from the last valid sample to
//           PM + 3 entries behind sample L - 1 (PM: p rounded up to an order class).  Eight samples per
//           lane and round, read as pitch.hip reads them; the clamped table sits in LDS once per workgroup
//   lags    on the vector ALU.  A lane takes four consecutive samples i .. i+3 per round and reads
//           z[i .. i+3+PM] as 16-byte LDS loads: 4 (PM + 1) multiply-adds on 4 + PM values held in
//           registers, lag tau in its own int64 accumulator (v_mad_i64_i32).
//   reduce  sixteen lags at a time through the image: lane (tau, q) adds the sixteen lanes 4 j + q of
//           lag tau, two cross-lane adds finish it, and the lanes with q = 0 write r as int64.
// No digits, no matrix cores and so no frame that needs a fallback: the workspace's counter is 0.
// (The forms that were measured against this one and dropped -- fp64 accumulators, the i8 matrix cores --
// are in DESIGN.md §4.12.)
//
// lpc_solve: a thread per row, a and the cepstrum in LDS columns (one per thread, so the triangular
// loops index LDS and no private array), R converted from the row of r at every use.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "dsp_audiorec.h"
#include "crop_frames.h"

namespace dsp {

constexpr int LPC_LMAX = 4096;
constexpr int LPC_PMAX = 32;
constexpr int LPC_QMAX = 64;
constexpr int LPC_RED_STRIDE = 68;  // accumulators per lag row of the reduction: 64 + 4, so that the rows
                                    // of the sixteen lags of a pass start four 8-byte banks apart
constexpr int LPC_SOLVE_THREADS = 64;

static bool lpc_in_plan(int B, int64_t max_len, int L, int S, int p)
{
    return B >= 0 && max_len >= 1 && L >= 2 && L <= LPC_LMAX && S >= 1 && p >= 1 && p <= LPC_PMAX && p <= L - 1;
}

// the order class: lags 0 .. PM are summed, PM a multiple of 4
static int lpc_order_class(int p) { return p <= 16 ? (p + 3) & ~3 : (p <= 24 ? 24 : 32); }

// entries of a wave's z image (a multiple of 8, at least L + 3 + PM) and of the table's copy, and the bytes
// of a wave's LDS region (the image, or the reduction's 16 rows)
static int lpc_image_len(int L, int PM) { return (L + 3 + PM + 7) & ~7; }
static size_t lpc_region_bytes(int L, int PM)
{
    return std::max<size_t>((size_t)lpc_image_len(L, PM) * 4, (size_t)16 * LPC_RED_STRIDE * sizeof(long long));
}

template <int PM>
__global__ __launch_bounds__(CROP_WAVES * 64) void lpc_autocorr(
    const int16_t *__restrict__ pcm, const int64_t *__restrict__ offsets, int64_t max_len, int L, int S, int p,
    const int32_t *__restrict__ window, const int32_t *__restrict__ start_end, int se_stride,
    const int32_t *__restrict__ n_frames, const int32_t *__restrict__ status, int row_stride, int64_t *__restrict__ r,
    int ld, int zlen, int region, unsigned *plain_frames)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lpc_lds[];
    __shared__ long long red[CROP_WAVES];
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // wv: scalar
    if (b == 0 && tid == 0) plain_frames[0] = 0u;
    crop_clip clip;
    if (!crop_gate(clip, pcm, offsets, max_len, start_end, se_stride, n_frames, status, row_stride, ld)) return;
    // w, clamped, in front of the waves' regions (zlen entries, zeros behind L); the barrier inside
    // crop_clip_centre orders it before the first frame
    int *wt = (int *)lpc_lds;
    if (window)
        for (int i = tid; i < zlen; i += CROP_WAVES * 64) wt[i] = i < L ? std::min(std::max(window[i], 0), 32768) : 0;
    const int c = crop_clip_centre(clip.x, clip.N, tid, red);

    int *zi = (int *)(lpc_lds + (window ? (size_t)zlen * 4 : 0) + (size_t)wv * region);
    long long *rd = (long long *)zi;  // the reduction's rows, over the image once the lag sums have read it
    const int rt = lane >> 2, rq = lane & 3;

    for (int t = wv; t < clip.nf; t += CROP_WAVES) {
        const crop_frame fr = crop_frame_at(clip, t, L, S);
        for (int i8 = lane * 8; i8 < zlen; i8 += 512) {
            int y[8];
            // zeros behind the valid samples
            crop_frame_load8(pcm, fr.f, fr.e_first, fr.odd, i8, fr.n, clip.total, c, y);
            if (window) {
                const crop_v4i w0 = *(const crop_v4i *)(wt + i8), w1 = *(const crop_v4i *)(wt + i8 + 4);
                // |y w + 16384| <= 65535 * 32768 + 16384 < 2^31
#pragma unroll
                for (int k = 0; k < 8; k++) y[k] = (y[k] * (k < 4 ? w0[k & 3] : w1[k & 3]) + 16384) >> 15;
            }
            *(crop_v4i *)(zi + i8) = crop_v4i{y[0], y[1], y[2], y[3]};
            *(crop_v4i *)(zi + i8 + 4) = crop_v4i{y[4], y[5], y[6], y[7]};
        }
        crop_publish();  // the image is this wave's own

        long long acc[PM + 1];
#pragma unroll
        for (int tau = 0; tau <= PM; tau++) acc[tau] = 0;
        // i0 <= L - 1, so the last entry read is i0 + 3 + PM < zlen
        for (int i0 = 4 * lane; i0 < fr.n; i0 += 256) {
            int v[4 + PM];
#pragma unroll
            for (int q = 0; q < 1 + PM / 4; q++) {
                const crop_v4i w = *(const crop_v4i *)(zi + i0 + 4 * q);
#pragma unroll
                for (int u = 0; u < 4; u++) v[4 * q + u] = w[u];
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int tau = 0; tau <= PM; tau++) acc[tau] += (long long)v[u] * v[u + tau];
        }

        const int64_t o = (b * ld + t) * (int64_t)(p + 1);
#pragma unroll
        for (int base = 0; base <= PM; base += 16) {
            crop_retire();  // the image (or the last pass's rows) has been read before it is overwritten
#pragma unroll
            for (int u = 0; u < 16; u++)
                if (base + u <= PM) rd[u * LPC_RED_STRIDE + lane] = acc[base + u];
            crop_publish();
            long long s = 0;
            if (base + rt <= PM) {
#pragma unroll
                for (int j = 0; j < 16; j++) s += rd[rt * LPC_RED_STRIDE + 4 * j + rq];
            }
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            if (rq == 0 && base + rt <= p) r[o + base + rt] = s;
        }
        crop_retire();  // the next frame's image is written only after this frame's reads
    }
}

#pragma clang fp contract(off)
// a_j at a[j * T], c_q at c[q * T]: this thread's columns of the two LDS tables (row 0 of each unused)
__global__ __launch_bounds__(LPC_SOLVE_THREADS) void lpc_solve(const int64_t *__restrict__ r, int64_t n, int p, int Q,
                                                               double *__restrict__ a_out, double *__restrict__ k_out,
                                                               double *__restrict__ err, int32_t *__restrict__ reached,
                                                               double *__restrict__ cep)
{
    extern __shared__ double lpc_cols[];
    constexpr int T = LPC_SOLVE_THREADS;
    const int64_t row = (int64_t)blockIdx.x * T + threadIdx.x;
    if (row >= n) return;  // no barrier below: a thread touches its own columns only
    double *a = lpc_cols + threadIdx.x, *c = lpc_cols + (size_t)(p + 1) * T + threadIdx.x;
    const int64_t *rr = r + row * (p + 1);
    double *ko = k_out + row * p;
    for (int j = 1; j <= p; j++) {
        a[j * T] = 0.0;
        ko[j - 1] = 0.0;
    }
    double E = (double)rr[0];
    int m = 0;
    for (int i = 1; i <= p; i++) {
        if (!(E > 0.0)) break;
        double acc = (double)rr[i];
        for (int j = 1; j < i; j++) acc = acc - a[j * T] * (double)rr[i - j];
        const double ki = acc / E;
        if (!(__builtin_fabs(ki) < 1.0)) break;
        // a'[j] and a'[i - j] need a[j] and a[i - j] only: the pair is replaced in place
        for (int j = 1; 2 * j <= i - 1; j++) {
            const double u = a[j * T], v = a[(i - j) * T];
            a[j * T] = u - ki * v;
            a[(i - j) * T] = v - ki * u;
        }
        if ((i & 1) == 0) {
            const double u = a[(i / 2) * T];
            a[(i / 2) * T] = u - ki * u;
        }
        a[i * T] = ki;
        ko[i - 1] = ki;
        E = E * (1.0 - ki * ki);
        m = i;
    }
    err[row] = E;
    reached[row] = m;
    for (int j = 1; j <= p; j++) a_out[row * p + j - 1] = a[j * T];
    for (int nn = 1; nn <= Q; nn++) {
        double s = 0.0;
        for (int q = nn - p > 1 ? nn - p : 1; q < nn; q++) s = s + ((double)q * c[q * T]) * a[(nn - q) * T];
        const double v = (nn <= p ? a[nn * T] : 0.0) + s / (double)nn;
        c[nn * T] = v;
        cep[row * Q + nn - 1] = v;
    }
}
#pragma clang fp contract(on)

template <int PM>
static hipError_t lpc_launch(int B, size_t lds, hipStream_t s, const int16_t *pcm, const int64_t *offsets, int64_t max_len,
                             int L, int S, int p, const int32_t *window, const int32_t *start_end, int se_stride,
                             const int32_t *n_frames, const int32_t *status, int row_stride, int64_t *r, int ld,
                             int zlen, int region, unsigned *counter)
{
    if (lds > 65536) {  // L above 3200 or so: past the default limit of dynamic LDS
        const hipError_t e = hipFuncSetAttribute((const void *)lpc_autocorr<PM>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lpc_autocorr<PM>, dim3((unsigned)B), dim3(CROP_WAVES * 64), lds, s, pcm, offsets, max_len, L, S,
                       p, window, start_end, se_stride, n_frames, status, row_stride, r, ld, zlen, region, counter);
    return hipGetLastError();
}

}  // namespace dsp

extern "C" size_t dsp_lpc_workspace_bytes(int B, int64_t max_len, int frame_length, int frame_shift, int order)
{
    return dsp::lpc_in_plan(B, max_len, frame_length, frame_shift, order) ? 256 : 0;
}

extern "C" int dsp_lpc_autocorr(const int16_t *pcm, const int64_t *offsets, int B, int64_t max_len, int frame_length,
                                int frame_shift, int order, const int32_t *window, const int32_t *start_end,
                                const int32_t *n_frames, const int32_t *status, int out_stride, int64_t *r, int ld,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    if (!dsp::lpc_in_plan(B, max_len, frame_length, frame_shift, order)) return DSP_ERR_ARGS;
    const bool outputs_ok = r && !((uintptr_t)r & 7) && !((uintptr_t)window & 3);
    int se, rs, rc;
    if (!dsp::crop_host_checks(B, ld, out_stride, pcm, offsets, start_end, n_frames, status, outputs_ok, workspace,
                               workspace_bytes, &se, &rs, &rc))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const int PM = dsp::lpc_order_class(order);
    const int zlen = dsp::lpc_image_len(frame_length, PM);
    const int region = (int)((dsp::lpc_region_bytes(frame_length, PM) + 15) & ~(size_t)15);
    const size_t lds = (window ? (size_t)zlen * 4 : 0) + (size_t)dsp::CROP_WAVES * region;  // at most 81 KiB
    hipError_t e;
#define LPC_CASE(P)                                                                                                   \
    case P:                                                                                                           \
        e = dsp::lpc_launch<P>(B, lds, s, pcm, offsets, max_len, frame_length, frame_shift, order, window, start_end, \
                               se, n_frames, status, rs, r, ld, zlen, region, (unsigned *)workspace);                      \
        break;
    switch (PM) {
        LPC_CASE(4)
        LPC_CASE(8)
        LPC_CASE(12)
        LPC_CASE(16)
        LPC_CASE(24)
    default:
        LPC_CASE(32)
    }
#undef LPC_CASE
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
}

extern "C" int dsp_lpc_solve(const int64_t *r, int64_t n, int order, int n_cep, double *a, double *k, double *err,
                             int32_t *reached, double *cep, void *stream)
{
    if (order < 1 || order > dsp::LPC_PMAX || n_cep < 0 || n_cep > dsp::LPC_QMAX || n < 0 || n > INT32_MAX)
        return DSP_ERR_ARGS;
    if (n == 0) return DSP_OK;
    if (!r || !a || !k || !err || !reached || (n_cep > 0 && !cep)) return DSP_ERR_ARGS;
    if (((uintptr_t)r & 7) || ((uintptr_t)a & 7) || ((uintptr_t)k & 7) || ((uintptr_t)err & 7) ||
        ((uintptr_t)reached & 3) || ((uintptr_t)cep & 7))
        return DSP_ERR_ARGS;
    constexpr int T = dsp::LPC_SOLVE_THREADS;
    const size_t lds = (size_t)(order + n_cep + 2) * T * sizeof(double);  // at most 49 KiB
    hipLaunchKernelGGL(dsp::lpc_solve, dim3((unsigned)((n + T - 1) / T)), dim3(T), lds, (hipStream_t)stream, r, n, order,
                       n_cep, a, k, err, reached, cep);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
}
