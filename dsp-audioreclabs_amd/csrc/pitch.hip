// pitch.hip -- dsp_pitch_track: the exact short-time autocorrelation and its argmax lag per crop frame
// (include/dsp_audiorec.h).  Every result is an exact integer.
//
// One workgroup of four waves per clip.  The workgroup sums the clip (the centring value c), then each
// wave takes every fourth frame of the crop on its own:
//   stage   y = x - c of the frame split into balanced byte digits y = 256 h + l, written as two byte
//           planes to the wave's own LDS image, zeros in front of the frame and behind its last valid
//           sample; r(0) is summed on the way in int64
//   lags    on the i8 matrix cores.  For a step of 64 samples from i0 and a tile of 256 lags from T,
//             A[m][k] = f[i0 + k - m]          B[k][n] = f[i0 + k + T + 16 n]
//           so D[m][n] collects the products at lag T + 16 n + m.  Both operands are runs of 16 bytes of
//           the same image: B's are 16-byte aligned (T is a multiple of 16), A's start m bytes early and
//           are funnelled out of five aligned words.  Three digit pairs (hh, hl + lh, ll) accumulate in
//           int32 -- at most 2 * 4096 * 2^14 = 2^27 -- and are recombined in int64.  A and B take their k
//           from the lane group and the byte in the same way, so any order the hardware sums k in is the
//           same for both; steps whose B lies wholly behind the frame are skipped.
//   plain   a frame with a sample whose h is no int8 (y >= 32640 or y < -32896: a full-scale sample, or a
//           large c) takes one lag per lane straight from memory in int64 instead.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "dsp_audiorec.h"
#include "crop_frames.h"

namespace dsp {

constexpr int PITCH_LMAX = 4096;
constexpr int PITCH_HEAD = 16;   // zero bytes in front of a plane: A reads up to 15 bytes before a step
constexpr int PITCH_TAIL = 336;  // bytes behind sample L - 1: a kept step's B reads at most 303 past it
constexpr int PITCH_TILES = 3;   // lag tiles that share one A fragment (36 accumulator registers)

static inline int pitch_plane_bytes(int L) { return (PITCH_HEAD + L + PITCH_TAIL + 15) & ~15; }

static bool pitch_in_plan(int B, int64_t max_len, int L, int S, int lag_min, int lag_max)
{
    return B >= 0 && max_len >= 1 && L >= 2 && L <= PITCH_LMAX && S >= 1 && lag_min >= 1 && lag_min <= lag_max &&
           lag_max <= L - 1;
}

// the larger value, the smaller lag among equals
__device__ __forceinline__ void pitch_better(long long &bv, int &bl, long long v, int l)
{
    if (v > bv || (v == bv && l < bl)) {
        bv = v;
        bl = l;
    }
}

// sixteen bytes from byte address a of a plane (a >= 1, any alignment) as an MFMA operand
__device__ __forceinline__ crop_v4i pitch_load_shifted(const unsigned char *plane, int a)
{
    const uint32_t *p = (const uint32_t *)(plane + (a & ~3));
    uint32_t w[5];
#pragma unroll
    for (int q = 0; q < 5; q++) w[q] = p[q];
    crop_v4i r;
#pragma unroll
    for (int q = 0; q < 4; q++) r[q] = (int)__builtin_amdgcn_alignbyte(w[q + 1], w[q], (uint32_t)(a & 3));
    return r;
}

// one step of 64 samples for NT lag tiles: A at byte a - col of the planes (shared by the tiles), tile u's
// B at byte bo + 256 u; every load is issued before the first MFMA
template <int NT>
__device__ __forceinline__ void pitch_step(const unsigned char *lo, const unsigned char *hi, int a, int col, int bo,
                                           crop_v4i (&hh)[PITCH_TILES], crop_v4i (&mid)[PITCH_TILES],
                                           crop_v4i (&ll)[PITCH_TILES])
{
    const crop_v4i al = pitch_load_shifted(lo, a - col), ah = pitch_load_shifted(hi, a - col);
    crop_v4i bl[NT], bh[NT];
#pragma unroll
    for (int u = 0; u < NT; u++) {
        bl[u] = *(const crop_v4i *)(lo + bo + 256 * u);
        bh[u] = *(const crop_v4i *)(hi + bo + 256 * u);
    }
#pragma unroll
    for (int u = 0; u < NT; u++) hh[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bh[u], hh[u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < NT; u++) ll[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bl[u], ll[u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < NT; u++) mid[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bl[u], mid[u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < NT; u++) mid[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bh[u], mid[u], 0, 0, 0);
}

__global__ void pitch_begin(unsigned *counters)
{
    counters[0] = 0u;
}

__global__ __launch_bounds__(CROP_WAVES * 64) void pitch_track(
    const int16_t *__restrict__ pcm, const int64_t *__restrict__ offsets, int64_t max_len, int L, int S, int lag_min,
    int lag_max, const int32_t *__restrict__ start_end, int se_stride, const int32_t *__restrict__ n_frames,
    const int32_t *__restrict__ status, int row_stride, int32_t *__restrict__ lag, int64_t *__restrict__ peak,
    int64_t *__restrict__ r0, int ld, int plane, unsigned *plain_frames)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char pitch_lds[];
    __shared__ long long red[CROP_WAVES];
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // wv: scalar
    crop_clip clip;
    if (!crop_gate(clip, pcm, offsets, max_len, start_end, se_stride, n_frames, status, row_stride, ld)) return;

    const int c = crop_clip_centre(clip.x, clip.N, tid, red);  // floor((2 sum + N) / (2 N))

    unsigned char *lo = pitch_lds + (size_t)wv * 2 * plane, *hi = lo + plane;
    if (lane < PITCH_HEAD / 4) {
        ((uint32_t *)lo)[lane] = 0u;
        ((uint32_t *)hi)[lane] = 0u;
    }
    const int img = plane - PITCH_HEAD;  // a multiple of 16
    const int tau0 = lag_min & ~15, ntile = (lag_max - tau0) / 256 + 1;
    const int col = lane & 15, grp = lane >> 4;

    for (int t = wv; t < clip.nf; t += CROP_WAVES) {
        const crop_frame fr = crop_frame_at(clip, t, L, S);
        long long e0 = 0;
        bool wide = false;
        // eight samples per lane and round (crop_frame_load8)
        for (int i8 = lane * 8; i8 < img; i8 += 512) {
            int y[8];
            crop_frame_load8(pcm, fr.f, fr.e_first, fr.odd, i8, fr.n, clip.total, c, y);
            uint32_t pl[2] = {0u, 0u}, ph[2] = {0u, 0u};
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int dl = ((y[k] + 128) & 255) - 128, dh = (y[k] - dl) >> 8;
                wide |= dh < -128 || dh > 127;
                e0 += (long long)y[k] * y[k];
                pl[k >> 2] |= (uint32_t)(dl & 255) << (8 * (k & 3));
                ph[k >> 2] |= (uint32_t)(dh & 255) << (8 * (k & 3));
            }
            *(uint2 *)(lo + PITCH_HEAD + i8) = make_uint2(pl[0], pl[1]);
            *(uint2 *)(hi + PITCH_HEAD + i8) = make_uint2(ph[0], ph[1]);
        }
        e0 = crop_wave_sum(e0);
        crop_publish();  // the image is this wave's own

        long long bv = INT64_MIN;
        int bl = INT32_MAX;
        if (__any(wide)) {
            for (int tau = lag_min + lane; tau <= lag_max; tau += 64) {
                long long r = 0;
                for (int i = 0; i + tau < fr.n; i++)
                    r += (long long)((int)fr.f[i] - c) * (long long)((int)fr.f[i + tau] - c);
                pitch_better(bv, bl, r, tau);
            }
            if (lane == 0) atomicAdd(plain_frames, 1u);
        } else {
            for (int tg = 0; tg < ntile; tg += PITCH_TILES) {
                const int base = tau0 + 256 * tg;
                crop_v4i hh[PITCH_TILES], mid[PITCH_TILES], ll[PITCH_TILES];
#pragma unroll
                for (int u = 0; u < PITCH_TILES; u++) hh[u] = mid[u] = ll[u] = crop_v4i{0, 0, 0, 0};
                // tile u's steps end where its B starts behind the frame (i0 + base + 256 u >= fr.n), so the
                // steps run with three tiles first, then two, then one: no condition inside a step
                const int nt = ntile - tg < PITCH_TILES ? ntile - tg : PITCH_TILES;
                const int a0 = PITCH_HEAD + 16 * grp, b0 = a0 + base + 16 * col;
                int i0 = 0;
                if (nt >= 3)
                    for (; i0 + base + 512 < fr.n; i0 += 64) pitch_step<3>(lo, hi, a0 + i0, col, b0 + i0, hh, mid, ll);
                if (nt >= 2)
                    for (; i0 + base + 256 < fr.n; i0 += 64) pitch_step<2>(lo, hi, a0 + i0, col, b0 + i0, hh, mid, ll);
                for (; i0 + base < fr.n; i0 += 64) pitch_step<1>(lo, hi, a0 + i0, col, b0 + i0, hh, mid, ll);
#pragma unroll
                for (int u = 0; u < PITCH_TILES; u++) {
                    if (tg + u < ntile) {
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            // D[m][n]: n on the lane's low four bits, m = 4 (lane >> 4) + r
                            const int tau = base + 256 * u + 16 * col + 4 * grp + r;
                            const long long v = 65536ll * hh[u][r] + 256ll * mid[u][r] + ll[u][r];
                            if (tau >= lag_min && tau <= lag_max) pitch_better(bv, bl, v, tau);
                        }
                    }
                }
            }
        }
        for (int m = 32; m; m >>= 1) {
            const long long ov = __shfl_xor(bv, m, 64);
            const int ol = __shfl_xor(bl, m, 64);
            pitch_better(bv, bl, ov, ol);
        }
        if (lane == 0) {
            const int64_t o = b * ld + t;
            lag[o] = bl;
            peak[o] = bv;
            r0[o] = e0;
        }
        crop_retire();  // the next frame's image is written only after this frame's reads
    }
}

}  // namespace dsp

extern "C" size_t dsp_pitch_workspace_bytes(int B, int64_t max_len, int frame_length, int frame_shift, int lag_min,
                                            int lag_max)
{
    return dsp::pitch_in_plan(B, max_len, frame_length, frame_shift, lag_min, lag_max) ? 256 : 0;
}

extern "C" int dsp_pitch_track(const int16_t *pcm, const int64_t *offsets, int B, int64_t max_len, int frame_length,
                               int frame_shift, int lag_min, int lag_max, const int32_t *start_end,
                               const int32_t *n_frames, const int32_t *status, int out_stride, int32_t *lag,
                               int64_t *peak, int64_t *r0, int ld, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!dsp::pitch_in_plan(B, max_len, frame_length, frame_shift, lag_min, lag_max)) return DSP_ERR_ARGS;
    const bool outputs_ok = lag && peak && r0 && !((uintptr_t)peak & 7) && !((uintptr_t)r0 & 7);
    int se_stride, row_stride, rc;
    if (!dsp::crop_host_checks(B, ld, out_stride, pcm, offsets, start_end, n_frames, status, outputs_ok, workspace,
                               workspace_bytes, &se_stride, &row_stride, &rc))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const int plane = dsp::pitch_plane_bytes(frame_length);
    const size_t lds = (size_t)dsp::CROP_WAVES * 2 * plane;  // at most 36 KiB
    hipLaunchKernelGGL(dsp::pitch_begin, dim3(1), dim3(1), 0, s, (unsigned *)workspace);
    hipLaunchKernelGGL(dsp::pitch_track, dim3((unsigned)B), dim3(dsp::CROP_WAVES * 64), lds, s, pcm, offsets, max_len,
                       frame_length, frame_shift, lag_min, lag_max, start_end, se_stride, n_frames, status, row_stride,
                       lag, peak, r0, ld, plane, (unsigned *)workspace);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
}
