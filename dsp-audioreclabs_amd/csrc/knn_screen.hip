// knn_screen.hip -- the fp32 stages of the exact KNN (pipeline: knn.hip): conversion, the three
// screens, and the pilot and seeds of the matrix-core screen, each with its host launcher.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsp_device.h"
#include "knn_internal.h"

namespace dsp {

static constexpr int KNN_RU = 4;  // rows x queries per unrolled step of the screen

// mode 0: plain rows (v, 0 ...); mode 1 (reference, expanded form): (-2 v, 0 ..., |v|^2);
// mode 2 (query, expanded form): (v, 0 ..., 1) -- so that |q - r|^2 = |q|^2 + q'.r'.
// One thread per row, its columns in chunks of 16 loaded together before any is used (the loads
// of a rolled column loop waited for each other: 16.9 us for 12 500 rows as for 100 000).
__global__ void knn_convert(const double *__restrict__ src, int64_t N, int D, int DP, int mode,
                            float *__restrict__ dst, unsigned int *maxnorm_bits)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float nrm = 0.f;
    if (i < N) {
        double n64 = 0.0;
        for (int c0 = 0; c0 < DP; c0 += 16) {
            double x[16];
#pragma unroll
            for (int c = 0; c < 16; c++) x[c] = c0 + c < D ? src[i * D + c0 + c] : 0.0;
#pragma unroll
            for (int c = 0; c < 16; c++) {
                const float v = (float)x[c];
                nrm = fmaf(v, v, nrm);
                n64 = fma(x[c], x[c], n64);
                float o = v;
                if (mode == 1) o = c0 + c < D ? (float)(-2.0 * x[c]) : 0.f;
                if (mode == 2 && c0 + c == DP - 1) o = 1.f;
                dst[i * DP + c0 + c] = o;
            }
        }
        if (mode == 1) dst[i * DP + DP - 1] = (float)n64;
    }
    // block max -> one atomic (non-negative floats order like their bit patterns)
    for (int o = 32; o > 0; o >>= 1) nrm = fmaxf(nrm, __shfl_xor(nrm, o, 64));
    if ((threadIdx.x & 63) == 0 && maxnorm_bits) atomicMax(maxnorm_bits, __float_as_uint(nrm));
}

// insert (d, r) into the ascending list (dl, il) of length KC if it beats the last entry:
// branch-free, dl'[i] = med3(dl[i-1], d, dl[i]) (an entry shifts down, takes d, or stays)
template <int KC>
__device__ __forceinline__ void topk_insert(float (&dl)[KC], int (&il)[KC], float d, int r)
{
    if (!(d < dl[KC - 1])) return;
    bool c[KC];
#pragma unroll
    for (int i = 0; i < KC; i++) c[i] = d < dl[i];
#pragma unroll
    for (int i = KC - 1; i > 0; i--) {
        il[i] = c[i - 1] ? il[i - 1] : (c[i] ? r : il[i]);
        dl[i] = __builtin_amdgcn_fmed3f(dl[i - 1], d, dl[i]);
    }
    il[0] = c[0] ? r : il[0];
    dl[0] = fminf(d, dl[0]);
}

// Direct form sum (q - r)^2 on the VALU, for D = 16 and D = 32 (no spare column for the expanded
// form of knn_screen_mfma).  QP queries per thread (queries q0 + tid + KNN_TQ * p): every 16-B LDS
// read of a reference row feeds QP FMA chains -- a broadcast ds_read_b128 costs the CU's LDS pipe
// 4 cycles, shared by 4 SIMDs, so at one query per thread the screen is LDS-bound
template <int DP, int KC, int QP>
__global__ __launch_bounds__(KNN_TQ) void knn_screen(const float *__restrict__ ref32, int64_t Nr,
                                                      const float *__restrict__ q32, int64_t Nq,
                                                      int64_t self_offset, int nsplit,
                                                      float *__restrict__ cand_d,
                                                      int *__restrict__ cand_i)
{
    __shared__ __attribute__((aligned(16))) float tile[KNN_TR * DP];
    const int qb = blockIdx.x, sp = blockIdx.y;
    const int tid = threadIdx.x;
    const int64_t per = (Nr + nsplit - 1) / nsplit;
    const int64_t r0 = (int64_t)sp * per, r1 = min(Nr, r0 + per);
    int64_t q[QP], self[QP];
    float qv[QP][DP];
    float dl[QP][KC];
    int il[QP][KC];
#pragma unroll
    for (int p = 0; p < QP; p++) {
        q[p] = (int64_t)qb * KNN_TQ * QP + tid + KNN_TQ * p;
#pragma unroll
        for (int c = 0; c < DP; c++) qv[p][c] = q[p] < Nq ? q32[q[p] * DP + c] : 0.f;
        self[p] = (self_offset >= 0 && q[p] < Nq) ? self_offset + q[p] : -1;
#pragma unroll
        for (int i = 0; i < KC; i++) {
            dl[p][i] = INFINITY;
            il[p][i] = -1;
        }
    }
    for (int64_t t0 = r0; t0 < r1; t0 += KNN_TR) {
        const int nt = (int)min((int64_t)KNN_TR, r1 - t0);
        __syncthreads();
        // cooperative tile load: KNN_TR rows x DP floats, float4 granules
        for (int e = tid; e < KNN_TR * DP / 4; e += KNN_TQ) {
            const int row = e / (DP / 4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < nt) v = reinterpret_cast<const float4 *>(ref32 + (t0 + row) * DP)[e % (DP / 4)];
            reinterpret_cast<float4 *>(tile)[e] = v;
        }
        __syncthreads();
        // rows in groups of RU: independent FMA chains, then the inserts in row order
        constexpr int RU = KNN_RU / QP > 0 ? KNN_RU / QP : 1;
        for (int j0 = 0; j0 < nt; j0 += RU) {
            float d[RU][QP];
#pragma unroll
            for (int u = 0; u < RU; u++) {
                const float4 *rv = reinterpret_cast<const float4 *>(tile + (j0 + u) * DP);  // rows >= nt are zero
#pragma unroll
                for (int p = 0; p < QP; p++) d[u][p] = 0.f;
#pragma unroll
                for (int c4 = 0; c4 < DP / 4; c4++) {
                    const float4 r = rv[c4];
#pragma unroll
                    for (int p = 0; p < QP; p++) {
                        float t;
                        t = qv[p][4 * c4 + 0] - r.x; d[u][p] = fmaf(t, t, d[u][p]);
                        t = qv[p][4 * c4 + 1] - r.y; d[u][p] = fmaf(t, t, d[u][p]);
                        t = qv[p][4 * c4 + 2] - r.z; d[u][p] = fmaf(t, t, d[u][p]);
                        t = qv[p][4 * c4 + 3] - r.w; d[u][p] = fmaf(t, t, d[u][p]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < RU; u++) {
                const int64_t r = t0 + j0 + u;
#pragma unroll
                for (int p = 0; p < QP; p++)
                    if (j0 + u < nt && r != self[p]) topk_insert<KC>(dl[p], il[p], d[u][p], (int)r);
            }
        }
    }
#pragma unroll
    for (int p = 0; p < QP; p++)
        if (q[p] < Nq) {
            const size_t o = ((size_t)sp * Nq + q[p]) * KC;
#pragma unroll
            for (int i = 0; i < KC; i++) {
                cand_d[o + i] = dl[p][i];
                cand_i[o + i] = il[p][i];
            }
        }
}

// Expanded-form screen on the matrix cores (D < DP, DP = 16 or 32): per 16 reference rows x 16
// queries, DP / 4 v_mfma_f32_16x16x4_f32 accumulate |q|^2 + q'.r'.  Measured on gfx950 this is
// bit for bit a k-ordered fp32 fmaf chain (MI355X_MICROARCH.md), but the certification does not
// depend on it: knn_err_coeffs' bound covers any summation order inside each K = 4 block with up
// to one rounding per product and per addition (see there).  A operand = reference rows
// (lane l: row l & 15), B = queries (lane l: query l & 15), lane l's dimensions in MFMA j are
// 16 (j / 4) + 4 (l >> 4) + (j & 3): one 16-B read per 4 MFMAs.  Result lane l: query l & 15,
// rows 4 (l >> 4) + v, v = 0..3, so four lanes keep partial top-KC lists of each query.
// Keeping the lists is the expensive part (an insertion costs the whole wave whenever one lane
// makes one), so each 16-row step first compares its distances with the query's threshold -- the
// smallest of the four lists' last entries: a row at or above it cannot be among the KC nearest
// of the union -- and inserts only when some lane has a distance below it.  Padding rows carry an
// infinite |r|^2 (distance +inf); the query's own row (self_offset) is masked only in the steps
// that can hold one of the wave's 32 own rows.
__host__ __device__ constexpr int mq_stride(int DP) { return DP + 4; }  // conflict-free 16-B reads
typedef float mq_f4 __attribute__((ext_vector_type(4)));
// lane_xor_f (dsp_device.h): the value of lane ^ 16 / lane ^ 32 by the gfx950 permlane swaps

// The three pieces the screen and the pilot share.  (1) A wave's MQ_T query tiles, first query
// wq0: lane (col, rg) gets query q = wq0 + 16 t + col, its B fragments qb, |q|^2 as the VALU screen
// computes it (an fmaf chain over the real columns), and the query's own reference row (-1: none).
template <int DP, int MQ_T>
__device__ __forceinline__ void mq_load_queries(const float *__restrict__ q32, int64_t Nq, int64_t wq0, int col,
                                                int rg, int64_t self_offset, int64_t (&q)[MQ_T],
                                                float (&qb)[MQ_T][DP / 4], float (&qn)[MQ_T],
                                                int64_t (&self)[MQ_T])
{
#pragma unroll
    for (int t = 0; t < MQ_T; t++) {
        q[t] = wq0 + t * 16 + col;
        const float *qr = q32 + (q[t] < Nq ? q[t] : 0) * DP;
        float n = 0.f;
#pragma unroll
        for (int c = 0; c < DP - 1; c++) n = fmaf(qr[c], qr[c], n);
        qn[t] = n;
#pragma unroll
        for (int h = 0; h < DP / 16; h++) {
            const float4 v = *reinterpret_cast<const float4 *>(qr + 16 * h + 4 * rg);
            qb[t][4 * h] = v.x;
            qb[t][4 * h + 1] = v.y;
            qb[t][4 * h + 2] = v.z;
            qb[t][4 * h + 3] = v.w;
        }
        self[t] = (self_offset >= 0 && q[t] < Nq) ? self_offset + q[t] : -1;
    }
}
// (2) One LDS tile: rows t0 .. t0 + nt of a set whose row j is reference row j * rstride, padded to
// MQ_TR rows whose |r|^2 is +inf (distance +inf).  Barriers are the caller's.
template <int DP>
__device__ __forceinline__ void mq_stage_tile(float *tile, const float *__restrict__ ref32, int64_t t0, int nt,
                                              int rstride, int tid)
{
    for (int e = tid; e < MQ_TR * DP / 4; e += 64 * MQ_W) {
        const int row = e / (DP / 4), c4 = e % (DP / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < nt)
            v = reinterpret_cast<const float4 *>(ref32 + (t0 + row) * rstride * DP)[c4];
        else if (c4 == DP / 4 - 1)
            v.w = INFINITY;
        *reinterpret_cast<float4 *>(tile + row * mq_stride(DP) + 4 * c4) = v;
    }
}
// (3) One 16-row step, tile rows s0 .. s0 + 15 = set rows rb .. rb + 15: the A fragment, DP / 4
// MFMAs per query tile from C = |q|^2, and +inf for a query's own row -- looked for only when the
// step meets [slo, shi), the rows that can be one of the wave's own queries (wave-uniform).
template <int DP, int MQ_T>
__device__ __forceinline__ void mq_step(const float *tile, int s0, int64_t rb, int col, int rg,
                                        const float (&qb)[MQ_T][DP / 4], const float (&qn)[MQ_T],
                                        const int64_t (&self)[MQ_T], int64_t slo, int64_t shi,
                                        mq_f4 (&acc)[MQ_T])
{
    constexpr int NJ = DP / 4;
    float a[NJ];
#pragma unroll
    for (int h = 0; h < DP / 16; h++) {
        const float4 v = *reinterpret_cast<const float4 *>(tile + (s0 + col) * mq_stride(DP) + 16 * h + 4 * rg);
        a[4 * h] = v.x;
        a[4 * h + 1] = v.y;
        a[4 * h + 2] = v.z;
        a[4 * h + 3] = v.w;
    }
#pragma unroll
    for (int t = 0; t < MQ_T; t++) acc[t] = mq_f4{qn[t], qn[t], qn[t], qn[t]};
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
        for (int t = 0; t < MQ_T; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], qb[t][j], acc[t], 0, 0, 0);
    if (rb < shi && rb + 16 > slo)
        for (int t = 0; t < MQ_T; t++)
            for (int v = 0; v < 4; v++)
                if (rb + 4 * rg + v == self[t]) acc[t][v] = INFINITY;
}

// Seeded thresholds: with `seed` non-null each query's threshold starts at seed[q] instead of +inf
// (knn_pilot_mfma + knn_seed: an upper bound of the KC-th smallest distance of the whole set, from
// a strided sample of the reference rows), so a split no longer pays the list warm-up of a
// threshold at +inf -- nearly every 16-row step inserting while the lists fill.  A row is kept only
// below min(seed, the lists' thresholds); knn_merge starts its screening cut-off at the seed, so a
// query whose seed was too tight fails certification and is answered by the exhaustive fallback:
// exactness never depends on the seed.
template <int DP, int KC>
__global__ __launch_bounds__(64 * MQ_W) void knn_screen_mfma(const float *__restrict__ ref32, int64_t Nr,
                                                           const float *__restrict__ q32, int64_t Nq,
                                                           int64_t self_offset, int nsplit,
                                                           float *__restrict__ cand_d, int *__restrict__ cand_i,
                                                           const float *__restrict__ seed)
{
    constexpr int MQ_T = mq_tiles(KC), MQ_QPB = mq_qpb(KC);
    __shared__ __attribute__((aligned(16))) float tile[MQ_TR * mq_stride(DP)];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, rg = lane >> 4;
    const int sp = blockIdx.y;
    const int64_t per = (Nr + nsplit - 1) / nsplit;
    const int64_t r0 = (int64_t)sp * per, r1 = min(Nr, r0 + per);
    const int64_t wq0 = (int64_t)blockIdx.x * MQ_QPB + wid * MQ_T * 16;  // the wave's first query
    // rows that can be one of the wave's own queries (self_offset >= 0): [slo, shi)
    const int64_t slo = self_offset >= 0 ? self_offset + wq0 : INT64_MIN / 2;
    const int64_t shi = self_offset >= 0 ? slo + 16 * MQ_T : INT64_MIN / 2;
    int64_t q[MQ_T], self[MQ_T];
    float qb[MQ_T][DP / 4], qn[MQ_T], tau[MQ_T];
    float dl[MQ_T][KC];
    int il[MQ_T][KC];
    mq_load_queries<DP, MQ_T>(q32, Nq, wq0, col, rg, self_offset, q, qb, qn, self);
#pragma unroll
    for (int t = 0; t < MQ_T; t++) {
        tau[t] = (seed && q[t] < Nq) ? seed[q[t]] : INFINITY;
#pragma unroll
        for (int i = 0; i < KC; i++) {
            dl[t][i] = INFINITY;
            il[t][i] = -1;
        }
    }
    for (int64_t t0 = r0; t0 < r1; t0 += MQ_TR) {
        const int nt = (int)min((int64_t)MQ_TR, r1 - t0);
        __syncthreads();
        mq_stage_tile<DP>(tile, ref32, t0, nt, 1, tid);
        __syncthreads();
        const int nt16 = (nt + 15) & ~15;
        for (int s0 = 0; s0 < nt16; s0 += 16) {
            const int64_t rb = t0 + s0;  // the step's first row
            mq_f4 acc[MQ_T];
            mq_step<DP, MQ_T>(tile, s0, rb, col, rg, qb, qn, self, slo, shi, acc);
            for (int t = 0; t < MQ_T; t++) {
                bool c[4];
#pragma unroll
                for (int v = 0; v < 4; v++) c[v] = acc[t][v] < tau[t];
                if (__builtin_amdgcn_ballot_w64(c[0] | c[1] | c[2] | c[3])) {
#pragma unroll
                    for (int v = 0; v < 4; v++)
                        if (c[v]) topk_insert<KC>(dl[t], il[t], acc[t][v], (int)(rb + 4 * rg + v));
                    float th = dl[t][KC - 1];
                    th = fminf(th, lane_xor_f(th, 16, lane));
                    th = fminf(th, lane_xor_f(th, 32, lane));
                    tau[t] = fminf(tau[t], th);  // = min(seed, the lists' thresholds)
                }
            }
        }
    }
    // the four partial lists of each query (lanes col, col + 16, col + 32, col + 48; disjoint
    // rows) -> one, by a butterfly over lane ^ 16 and lane ^ 32
#pragma unroll
    for (int t = 0; t < MQ_T; t++) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int m = 16 << h;
            float pd[KC];
            int pi[KC];
#pragma unroll
            for (int i = 0; i < KC; i++) {
                pd[i] = __shfl_xor(dl[t][i], m, 64);
                pi[i] = __shfl_xor(il[t][i], m, 64);
            }
#pragma unroll
            for (int i = 0; i < KC; i++)
                if (pi[i] >= 0) topk_insert<KC>(dl[t], il[t], pd[i], pi[i]);
        }
        if (rg == 0 && q[t] < Nq) {
            const size_t o = ((size_t)sp * Nq + q[t]) * KC;
#pragma unroll
            for (int i = 0; i < KC; i++) {
                cand_d[o + i] = dl[t][i];
                // never null; without the test the KC = 36 kernels are allocated 183 VGPRs for the
                // same instructions (two waves per SIMD) instead of 149 (three)
                if (cand_i) cand_i[o + i] = il[t][i];
            }
        }
    }
}

// The pilot (seeded thresholds): over the sampled rows (sample row j = reference row j * rstride)
// each query needs only an upper bound for the KC-th smallest distance of the whole set, and the
// KC-th smallest of any KC distinct rows' distances is one.  So instead of top-KC lists (whose
// insertions, from thresholds at +inf, were most of the old pilot's time) every lane keeps running
// minima: lane (col, rg) of a 16 x 16 MFMA tile sees rows rb + 4 rg + v, v = 0..3, and keeps one
// minimum per (v, step parity) -- PIL_CLS = 32 disjoint row classes per query and split, written
// to pilot_d[split][query][32]; knn_seed then takes the KC-th smallest of all of them, which is
// >= the KC-th smallest of the sample >= the KC-th smallest of the set.  Each class minimum over
// ~nsample / 32 rows sits near quantile 1/(nsample/32) of the query's distances, and the 6th of 32
// such near quantile 0.2 * 32 / nsample: as tight as the exact 6th smallest of the sample.
// Rows are numbered in the sample, so a query's own row is sample row self / rstride when rstride
// divides it, and in no step otherwise.
template <int DP>
__global__ __launch_bounds__(64 * MQ_W) void knn_pilot_mfma(const float *__restrict__ ref32, int64_t Nr,
                                                            const float *__restrict__ q32, int64_t Nq,
                                                            int64_t self_offset, int nsplit,
                                                            float *__restrict__ pilot_d, int rstride)
{
    constexpr int MQ_T = KNN_MQ_T, MQ_QPB = 16 * MQ_T * MQ_W;
    static_assert(MQ_TR % 32 == 0, "two 16-row steps per trip");
    static_assert(PIL_CLS == 32, "4 row groups x 2 step parities x 4 rows");
    __shared__ __attribute__((aligned(16))) float tile[MQ_TR * mq_stride(DP)];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, rg = lane >> 4;
    const int sp = blockIdx.y;
    const int64_t per = (Nr + nsplit - 1) / nsplit;  // Nr: rows of the sample
    const int64_t r0 = (int64_t)sp * per, r1 = min(Nr, r0 + per);
    const int64_t wq0 = (int64_t)blockIdx.x * MQ_QPB + wid * MQ_T * 16;
    const int64_t g0 = self_offset + wq0, g1 = g0 + 16 * MQ_T;
    const int64_t slo = self_offset >= 0 ? (g0 + rstride - 1) / rstride : INT64_MIN / 2;
    const int64_t shi = self_offset >= 0 ? (g1 + rstride - 1) / rstride : INT64_MIN / 2;
    int64_t q[MQ_T], self[MQ_T];
    float qb[MQ_T][DP / 4], qn[MQ_T], mn[MQ_T][2][4];
    mq_load_queries<DP, MQ_T>(q32, Nq, wq0, col, rg, self_offset, q, qb, qn, self);
#pragma unroll
    for (int t = 0; t < MQ_T; t++) {
        self[t] = (self[t] >= 0 && self[t] % rstride == 0) ? self[t] / rstride : -1;
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int v = 0; v < 4; v++) mn[t][h][v] = INFINITY;
    }
    for (int64_t t0 = r0; t0 < r1; t0 += MQ_TR) {
        const int nt = (int)min((int64_t)MQ_TR, r1 - t0);
        __syncthreads();
        mq_stage_tile<DP>(tile, ref32, t0, nt, rstride, tid);
        __syncthreads();
        const int nt32 = (nt + 31) & ~31;
        for (int s0 = 0; s0 < nt32; s0 += 32) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                mq_f4 acc[MQ_T];
                mq_step<DP, MQ_T>(tile, s0 + 16 * h, t0 + s0 + 16 * h, col, rg, qb, qn, self, slo, shi, acc);
#pragma unroll
                for (int t = 0; t < MQ_T; t++)
#pragma unroll
                    for (int v = 0; v < 4; v++) mn[t][h][v] = fminf(mn[t][h][v], acc[t][v]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < MQ_T; t++) {
        if (q[t] >= Nq) continue;
        float *o = pilot_d + ((size_t)sp * Nq + q[t]) * PIL_CLS + 8 * rg;
        *reinterpret_cast<float4 *>(o) = make_float4(mn[t][0][0], mn[t][0][1], mn[t][0][2], mn[t][0][3]);
        *reinterpret_cast<float4 *>(o + 4) = make_float4(mn[t][1][0], mn[t][1][1], mn[t][1][2], mn[t][1][3]);
    }
}

// the seed of each query: the KC-th smallest of the pilot's nsplit x PIL_CLS class minima, one
// thread per query
template <int KC>
__global__ __launch_bounds__(256) void knn_seed(const float *__restrict__ pilot_d, int nsplit, int64_t Nq,
                                                float *__restrict__ seed, float scale)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Nq) return;
    float k32[KC];
#pragma unroll
    for (int i = 0; i < KC; i++) k32[i] = INFINITY;
    for (int s = 0; s < nsplit; s++) {
        const float *c = pilot_d + ((size_t)s * Nq + q) * PIL_CLS;
#pragma unroll
        for (int i = 0; i < PIL_CLS; i++) {
            float v = c[i];
#pragma unroll
            for (int j = 0; j < KC; j++) {
                const float lo = fminf(v, k32[j]);
                v = fmaxf(v, k32[j]);
                k32[j] = lo;
            }
        }
    }
    seed[q] = k32[KC - 1] * scale;  // scale: 1 (< 1 only in the diagnostic build's tests)
}

// High-dimensional rows (D > 32: the sequence method's flattened (E, ZCR) sequences,
// compare_feature_methods.py:117-154): direct form sum (q - r)^2 in fp32, the dimensions walked
// in chunks of 16 against LDS tiles of 64 reference rows; one query per thread, 64 running
// distances in registers, then the same top-KC insertion.
static constexpr int HD_ROWS = 64, HD_COLS = 16;
template <int KC>
__global__ __launch_bounds__(KNN_TQ) void knn_screen_hd(const float *__restrict__ ref32, int64_t Nr,
                                                         const float *__restrict__ q32, int64_t Nq, int DP,
                                                         int64_t self_offset, int nsplit,
                                                         float *__restrict__ cand_d, int *__restrict__ cand_i)
{
    __shared__ __attribute__((aligned(16))) float tile[HD_ROWS * HD_COLS];
    const int tid = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * KNN_TQ + tid;
    const int sp = blockIdx.y;
    const int64_t per = (Nr + nsplit - 1) / nsplit;
    const int64_t r0 = (int64_t)sp * per, r1 = min(Nr, r0 + per);
    const int64_t self = (self_offset >= 0 && q < Nq) ? self_offset + q : -1;
    const float *qrow = q32 + (q < Nq ? q : 0) * DP;
    float dl[KC];
    int il[KC];
#pragma unroll
    for (int i = 0; i < KC; i++) {
        dl[i] = INFINITY;
        il[i] = -1;
    }
    for (int64_t t0 = r0; t0 < r1; t0 += HD_ROWS) {
        const int nt = (int)min((int64_t)HD_ROWS, r1 - t0);
        float d[HD_ROWS];
#pragma unroll
        for (int u = 0; u < HD_ROWS; u++) d[u] = 0.f;
        for (int c0 = 0; c0 < DP; c0 += HD_COLS) {
            float qc[HD_COLS];
#pragma unroll
            for (int c4 = 0; c4 < HD_COLS / 4; c4++) {
                const float4 v = reinterpret_cast<const float4 *>(qrow + c0)[c4];
                qc[4 * c4] = v.x;
                qc[4 * c4 + 1] = v.y;
                qc[4 * c4 + 2] = v.z;
                qc[4 * c4 + 3] = v.w;
            }
            __syncthreads();
            {  // 64 rows x 16 columns, one float4 per thread
                const int row = tid >> 2, c4 = tid & 3;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < nt) v = reinterpret_cast<const float4 *>(ref32 + (t0 + row) * DP + c0)[c4];
                reinterpret_cast<float4 *>(tile)[tid] = v;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < HD_ROWS; u++) {
                const float4 *rv = reinterpret_cast<const float4 *>(tile + u * HD_COLS);
#pragma unroll
                for (int c4 = 0; c4 < HD_COLS / 4; c4++) {
                    const float4 r = rv[c4];
                    float t;
                    t = qc[4 * c4 + 0] - r.x; d[u] = fmaf(t, t, d[u]);
                    t = qc[4 * c4 + 1] - r.y; d[u] = fmaf(t, t, d[u]);
                    t = qc[4 * c4 + 2] - r.z; d[u] = fmaf(t, t, d[u]);
                    t = qc[4 * c4 + 3] - r.w; d[u] = fmaf(t, t, d[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < HD_ROWS; u++) {
            const int64_t r = t0 + u;
            if (u < nt && r != self) topk_insert<KC>(dl, il, d[u], (int)r);
        }
    }
    if (q < Nq) {
        const size_t o = ((size_t)sp * Nq + q) * KC;
#pragma unroll
        for (int i = 0; i < KC; i++) {
            cand_d[o + i] = dl[i];
            cand_i[o + i] = il[i];
        }
    }
}

// ---- host launchers (knn_internal.h) ----
namespace {
template <class F>
void dispatch_dp(int DP, F &&f)  // the padded widths of D <= 32
{
    if (DP == 16) f(std::integral_constant<int, 16>{});
    if (DP == 32) f(std::integral_constant<int, 32>{});
}
unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
}  // namespace

void launch_knn_convert(hipStream_t s, const double *src, int64_t N, int D, int DP, int mode, float *dst,
                        unsigned int *maxnorm_bits)
{
    hipLaunchKernelGGL(knn_convert, dim3(blocks(N, 256)), dim3(256), 0, s, src, N, D, DP, mode, dst, maxnorm_bits);
}

void launch_knn_screen(hipStream_t s, int DP, int KC, int nsplit, const float *ref32, int64_t Nr, const float *q32,
                       int64_t Nq, int64_t self_offset, float *cand_d, int *cand_i)
{
    const dim3 g(blocks(Nq, KNN_TQ * KNN_QP), (unsigned)nsplit);
    dispatch_dp(DP, [&](auto dp) {
        dispatch_kc(KC, [&](auto kc) {
            if constexpr (kc() >= 8)  // KC = 6 is the matrix-core screen's alone
                hipLaunchKernelGGL((knn_screen<dp(), kc(), KNN_QP>), g, dim3(KNN_TQ), 0, s, ref32, Nr, q32, Nq,
                                   self_offset, nsplit, cand_d, cand_i);
        });
    });
}

void launch_knn_screen_hd(hipStream_t s, int DP, int KC, int nsplit, const float *ref32, int64_t Nr,
                          const float *q32, int64_t Nq, int64_t self_offset, float *cand_d, int *cand_i)
{
    const dim3 g(blocks(Nq, KNN_TQ), (unsigned)nsplit);
    dispatch_kc(KC, [&](auto kc) {
        if constexpr (kc() >= 8)
            hipLaunchKernelGGL((knn_screen_hd<kc()>), g, dim3(KNN_TQ), 0, s, ref32, Nr, q32, Nq, DP, self_offset,
                               nsplit, cand_d, cand_i);
    });
}

void launch_knn_screen_mfma(hipStream_t s, int DP, int KC, int nsplit, const float *ref32, int64_t Nr,
                            const float *q32, int64_t Nq, int64_t self_offset, float *cand_d, int *cand_i,
                            const float *seed)
{
    const dim3 g(blocks(Nq, mq_qpb(KC)), (unsigned)nsplit);
    dispatch_dp(DP, [&](auto dp) {
        dispatch_kc(KC, [&](auto kc) {
            hipLaunchKernelGGL((knn_screen_mfma<dp(), kc()>), g, dim3(64 * MQ_W), 0, s, ref32, Nr, q32, Nq,
                               self_offset, nsplit, cand_d, cand_i, seed);
        });
    });
}

void launch_knn_pilot(hipStream_t s, int DP, int nsplit_p, const float *ref32, int64_t nsample, int rstride,
                      const float *q32, int64_t Nq, int64_t self_offset, float *pilot_d)
{
    const dim3 g(blocks(Nq, 16 * KNN_MQ_T * MQ_W), (unsigned)nsplit_p);
    dispatch_dp(DP, [&](auto dp) {
        hipLaunchKernelGGL((knn_pilot_mfma<dp()>), g, dim3(64 * MQ_W), 0, s, ref32, nsample, q32, Nq, self_offset,
                           nsplit_p, pilot_d, rstride);
    });
}

void launch_knn_seed(hipStream_t s, int KC, const float *pilot_d, int nsplit_p, int64_t Nq, float *seed, float scale)
{
    dispatch_kc(KC, [&](auto kc) {
        hipLaunchKernelGGL((knn_seed<kc()>), dim3(blocks(Nq, 256)), dim3(256), 0, s, pilot_d, nsplit_p, Nq, seed,
                           scale);
    });
}

}  // namespace dsp
