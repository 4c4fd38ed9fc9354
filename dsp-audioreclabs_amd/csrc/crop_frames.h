// crop_frames.h -- what a crop-frame kernel is (pitch.hip: dsp_pitch_track, lpc.hip: dsp_lpc_autocorr): one
// workgroup of CROP_WAVES waves per clip, the gate that keeps it inside the clip, the clip sum behind the
// centring value c of include/dsp_audiorec.h, a frame's place in pcm and the loads of its samples, the two
// fences of a wave's own LDS image, and the argument checks of the two C entry points.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "dsp_audiorec.h"

namespace dsp {

constexpr int CROP_WAVES = 4;

typedef int crop_v4i __attribute__((ext_vector_type(4)));

// The entry points' shared checks, behind the plan's own.  false: *rc answers the call (B == 0 is DSP_OK
// with no pointer looked at).  outputs_ok: the caller's own pointers are there and aligned.
// se_stride and row_stride are the words between two clips' (start, end) pairs and n_frames / status.
static inline bool crop_host_checks(int B, int ld, int out_stride, const void *pcm, const void *offsets,
                                    const void *start_end, const void *n_frames, const void *status, bool outputs_ok,
                                    const void *workspace, size_t workspace_bytes, int *se_stride, int *row_stride,
                                    int *rc)
{
    *se_stride = out_stride ? out_stride : 2;
    *row_stride = out_stride ? out_stride : 1;
    *rc = DSP_ERR_ARGS;
    if (ld < 1 || (out_stride != 0 && out_stride < DSP_OUT_ROW_WORDS)) return false;
    if (B == 0) {
        *rc = DSP_OK;
        return false;
    }
    if (!pcm || !offsets || !start_end || !n_frames || !status || !outputs_ok || ((uintptr_t)pcm & 3)) return false;
    *rc = DSP_ERR_WORKSPACE;
    return workspace && workspace_bytes >= 256;
}

// workgroup blockIdx.x's clip x[0..N) at sample off of pcm (total samples), its crop [st, en) and its frame
// count, at most ld
struct crop_clip {
    const int16_t *x;
    int64_t off, N, st, en, total;
    int nf;
};

// false: the workgroup leaves the clip alone -- a failed status, or fields that would take a read outside
// the clip.  Every condition is uniform over the workgroup, so all its threads return together: the call
// stays ahead of the __syncthreads inside crop_clip_centre.
__device__ __forceinline__ bool crop_gate(crop_clip &c, const int16_t *__restrict__ pcm,
                                          const int64_t *__restrict__ offsets, int64_t max_len,
                                          const int32_t *__restrict__ start_end, int se_stride,
                                          const int32_t *__restrict__ n_frames, const int32_t *__restrict__ status,
                                          int row_stride, int ld)
{
    const int64_t b = blockIdx.x;
    if ((status[b * row_stride] & 0xFF) != 0) return false;
    c.off = offsets[b];
    c.N = offsets[b + 1] - c.off;
    c.st = start_end[b * se_stride];
    c.en = start_end[b * se_stride + 1];
    c.nf = n_frames[b * row_stride];
    if (c.N < 1 || c.N > max_len || c.st < 0 || c.en < c.st || c.en > c.N || c.nf < 1) return false;
    if (c.nf > ld) c.nf = ld;
    c.x = pcm + c.off;
    c.total = offsets[gridDim.x];  // pcm holds at least this many samples
    return true;
}

// frame t of the crop: L samples from f, the first n of them valid (zeros behind them); f[0] is sample
// e_first of pcm, odd = e_first & 1
struct crop_frame {
    const int16_t *f;
    int64_t e_first;
    int odd, n;
};

__device__ __forceinline__ crop_frame crop_frame_at(const crop_clip &c, int t, int L, int S)
{
    const int64_t fs = c.st + (int64_t)t * S;
    const int64_t left = c.en - fs;
    crop_frame fr;
    fr.f = c.x + fs;
    fr.e_first = c.off + fs;
    fr.odd = (int)(fr.e_first & 1);
    fr.n = left < 0 ? 0 : (left < L ? (int)left : L);
    return fr;
}

__device__ __forceinline__ long long crop_wave_sum(long long v)
{
    for (int m = 32; m; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// c = floor((2 sum + N) / (2 N)) of the clip x[0..N), N >= 1, by the whole workgroup (every thread calls
// it: one barrier inside); red: CROP_WAVES words of LDS.
// (the sum reads the whole clip once: 16-byte loads between the clip's first and last 16-byte
// boundary, single samples in front of and behind them -- nothing outside the clip)
__device__ __forceinline__ int crop_clip_centre(const int16_t *__restrict__ x, int64_t N, int tid, long long *red)
{
    const int64_t head = std::min<int64_t>(N, (int64_t)((16 - ((uintptr_t)x & 15)) & 15) / 2);
    const int64_t nvec = (N - head) / 8;
    const crop_v4i *xv = (const crop_v4i *)(x + head);
    long long s = 0;
    if (tid < head) s += x[tid];
    for (int64_t i = tid; i < nvec; i += CROP_WAVES * 64) {
        const crop_v4i v = xv[i];
        int part = 0;  // eight int16: no overflow
#pragma unroll
        for (int q = 0; q < 4; q++) part += (int)(int16_t)(v[q] & 0xffff) + (v[q] >> 16);
        s += part;
    }
    for (int64_t i = head + nvec * 8 + tid; i < N; i += CROP_WAVES * 64) s += x[i];
    s = crop_wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    s = 0;
    for (int q = 0; q < CROP_WAVES; q++) s += red[q];
    const long long num = 2 * s + N, den = 2 * N;
    long long cq = num / den;
    if (num % den != 0 && num < 0) cq--;
    return (int)cq;
}

// y[k] = f[i8 + k] - c for i8 + k < n, 0 behind the n valid samples of the frame f (sample e_first of
// pcm, odd = e_first & 1): as 32-bit words of pcm (funnelled by one sample when the frame starts on an odd
// one) where all eight are valid and the word behind them lies inside pcm (total samples), one by one
// at the frame's end
__device__ __forceinline__ void crop_frame_load8(const int16_t *__restrict__ pcm, const int16_t *__restrict__ f,
                                                 int64_t e_first, int odd, int i8, int n, int64_t total, int c,
                                                 int (&y)[8])
{
    if (i8 + 8 <= n && e_first + i8 + 8 < total) {
        const uint32_t *q = (const uint32_t *)pcm + ((e_first + i8 - odd) >> 1);
        uint32_t w[5];
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = q[k];
        w[4] = odd ? q[4] : 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t d = (uint32_t)((((uint64_t)w[k + 1] << 32) | w[k]) >> (16 * odd));
            y[2 * k] = (int)(int16_t)(d & 0xffffu) - c;
            y[2 * k + 1] = ((int)d >> 16) - c;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) y[k] = i8 + k < n ? (int)f[i8 + k] - c : 0;
    }
}

// The fences of a wave's own LDS region, which no other wave touches.
// publish-then-read: what the wave's lanes have written is ordered before what they read next
__device__ __forceinline__ void crop_publish()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// retire-before-overwrite: every lane has read the region before any lane writes it again
__device__ __forceinline__ void crop_retire()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

}  // namespace dsp
