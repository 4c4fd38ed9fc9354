// pitch_internal.h -- what pitch.hip (dsp_pitch_track) and lpc.hip (dsp_lpc_autocorr) share: the clip
// sum behind the centring value c of include/dsp_audiorec.h, one workgroup of PITCH_WAVES waves per clip,
// the loads of a frame's samples, and the unaligned operand load of the i8 matrix-core scheme.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace dsp {

constexpr int PITCH_WAVES = 4;

typedef int pitch_v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ long long pitch_wave_sum(long long v)
{
    for (int m = 32; m; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// c = floor((2 sum + N) / (2 N)) of the clip x[0..N), N >= 1, by the whole workgroup (every thread calls
// it: one barrier inside); red: PITCH_WAVES words of LDS.
// (the sum reads the whole clip once: 16-byte loads between the clip's first and last 16-byte
// boundary, single samples in front of and behind them -- nothing outside the clip)
__device__ __forceinline__ int pitch_clip_centre(const int16_t *__restrict__ x, int64_t N, int tid, long long *red)
{
    const int64_t head = std::min<int64_t>(N, (int64_t)((16 - ((uintptr_t)x & 15)) & 15) / 2);
    const int64_t nvec = (N - head) / 8;
    const pitch_v4i *xv = (const pitch_v4i *)(x + head);
    long long s = 0;
    if (tid < head) s += x[tid];
    for (int64_t i = tid; i < nvec; i += PITCH_WAVES * 64) {
        const pitch_v4i v = xv[i];
        int part = 0;  // eight int16: no overflow
#pragma unroll
        for (int q = 0; q < 4; q++) part += (int)(int16_t)(v[q] & 0xffff) + (v[q] >> 16);
        s += part;
    }
    for (int64_t i = head + nvec * 8 + tid; i < N; i += PITCH_WAVES * 64) s += x[i];
    s = pitch_wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    s = 0;
    for (int q = 0; q < PITCH_WAVES; q++) s += red[q];
    const long long num = 2 * s + N, den = 2 * N;
    long long cq = num / den;
    if (num % den != 0 && num < 0) cq--;
    return (int)cq;
}

// y[k] = f[i8 + k] - c for i8 + k < n, 0 behind the n valid samples of the frame f (sample e_first of
// pcm, odd = e_first & 1): as 32-bit words of pcm (funnelled by one sample when the frame starts on an odd
// one) where all eight are valid and the word behind them lies inside pcm (total samples), one by one
// at the frame's end
__device__ __forceinline__ void pitch_frame_load8(const int16_t *__restrict__ pcm, const int16_t *__restrict__ f,
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

// sixteen bytes from byte address a of a plane (a >= 1, any alignment) as an MFMA operand
__device__ __forceinline__ pitch_v4i pitch_load_shifted(const unsigned char *plane, int a)
{
    const uint32_t *p = (const uint32_t *)(plane + (a & ~3));
    uint32_t w[5];
#pragma unroll
    for (int q = 0; q < 5; q++) w[q] = p[q];
    pitch_v4i r;
#pragma unroll
    for (int q = 0; q < 4; q++) r[q] = (int)__builtin_amdgcn_alignbyte(w[q + 1], w[q], (uint32_t)(a & 3));
    return r;
}

}  // namespace dsp
