// knn_internal.h -- what the KNN translation units share: the launch-shape constants (the host's
// layout and split model in knn.hip must agree with the kernels in knn_screen.hip / knn_merge.hip)
// and the host launchers.  Every kernel is launched from the translation unit that defines it, so
// the objects link as plain C++ (no relocatable device code).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace dsp {

static constexpr int KNN_TQ = 256;   // queries per screening workgroup (one per thread)
static constexpr int KNN_TR = 256;   // reference rows per LDS tile
static constexpr int KNN_SLACK = 3;  // extra screened candidates per split (k = 5 -> 8)
#ifndef DSP_KNN_QP
#define DSP_KNN_QP 2
#endif
static constexpr int KNN_QP = DSP_KNN_QP;  // queries per screening thread (VALU screen, D = 16 / 32)

// matrix-core screen and pilot
#ifndef KNN_MQ_W
#define KNN_MQ_W 4
#endif
#ifndef KNN_MQ_T
#define KNN_MQ_T 2
#endif
#ifndef KNN_MQ_TR
#define KNN_MQ_TR 256
#endif
static constexpr int MQ_W = KNN_MQ_W;    // waves per workgroup
static constexpr int MQ_TR = KNN_MQ_TR;  // reference rows per LDS tile
// query tiles (16 queries) per wave: two while the lists are short, one for long lists (k > 13)
__host__ __device__ constexpr int mq_tiles(int KC) { return KC <= 16 ? KNN_MQ_T : 1; }
__host__ __device__ constexpr int mq_qpb(int KC) { return 16 * mq_tiles(KC) * MQ_W; }  // queries per workgroup
static constexpr int PIL_CLS = 32;  // the pilot's row classes (minima) per query and split

// merge
#ifndef KNN_MG
#define KNN_MG 8
#endif
static constexpr int MG = KNN_MG;  // lanes per query in knn_merge (a power of two <= 64)
static constexpr int KMAX = 32;    // largest k
// a query is certified only while |q|^2 + max |r|^2 < 2^125: no fp32 value of any screen then
// overflows (knn.hip, after knn_err_coeffs)
static constexpr double KNN_F32_SAFE = 0x1p125;  // 4.25e37; FLT_MAX is just under 2^128

// fallback
static constexpr int FB_T = 256;
static constexpr int FB_C = 64;        // queries on the partitioned scan
static constexpr int FB_PMAX = 64;     // parts per query (one lane per part in the final merge)
static constexpr int FB_PROWS = 1024;  // target rows per part

// f(std::integral_constant<int, KC>) for the candidate-list length the layout chose (pick_kc, or 6
// for the matrix-core screen over short splits); false when there is no such length
template <class F>
bool dispatch_kc(int KC, F &&f)
{
    switch (KC) {
    case 6: f(std::integral_constant<int, 6>{}); return true;
    case 8: f(std::integral_constant<int, 8>{}); return true;
    case 16: f(std::integral_constant<int, 16>{}); return true;
    case 24: f(std::integral_constant<int, 24>{}); return true;
    case 36: f(std::integral_constant<int, 36>{}); return true;
    }
    return false;
}

// ---- knn_screen.hip (grids follow from the constants above) ----
// mode 0: plain rows; 1: reference rows, expanded form; 2: query rows, expanded form
void launch_knn_convert(hipStream_t s, const double *src, int64_t N, int D, int DP, int mode, float *dst,
                        unsigned int *maxnorm_bits);
// D = 16 / 32 (knn_screen), D > 32 (knn_screen_hd), D < DP (knn_screen_mfma; seed may be null)
void launch_knn_screen(hipStream_t s, int DP, int KC, int nsplit, const float *ref32, int64_t Nr, const float *q32,
                       int64_t Nq, int64_t self_offset, float *cand_d, int *cand_i);
void launch_knn_screen_hd(hipStream_t s, int DP, int KC, int nsplit, const float *ref32, int64_t Nr,
                          const float *q32, int64_t Nq, int64_t self_offset, float *cand_d, int *cand_i);
void launch_knn_screen_mfma(hipStream_t s, int DP, int KC, int nsplit, const float *ref32, int64_t Nr,
                            const float *q32, int64_t Nq, int64_t self_offset, float *cand_d, int *cand_i,
                            const float *seed);
// class minima over the sample rows j * rstride, j < nsample, then each query's seed from them
void launch_knn_pilot(hipStream_t s, int DP, int nsplit_p, const float *ref32, int64_t nsample, int rstride,
                      const float *q32, int64_t Nq, int64_t self_offset, float *pilot_d);
void launch_knn_seed(hipStream_t s, int KC, const float *pilot_d, int nsplit_p, int64_t Nq, float *seed, float scale);

// ---- knn_merge.hip ----
// false when no merge kernel covers (KC, k): the layout broke KC >= k + KNN_SLACK
bool launch_knn_merge(hipStream_t s, int KC, const double *ref, const double *query, int64_t Nr, int64_t Nq, int D,
                      int k, int nsplit, int64_t self_offset, const float *cand_d, const int *cand_i,
                      const unsigned int *maxnorm_bits, double err_rel, double err_abs, const int32_t *labels,
                      int32_t *idx, double *dist, int32_t *pred, int *fb_count, int *fb_list, const float *seed);
// KM = 8 / 16 / 32 (the layout's fb_km), P parts per query for the first FB_C listed queries
void launch_knn_fallback(hipStream_t s, int KM, const double *ref, const double *query, int64_t Nr, int64_t Nq, int D,
                         int k, int64_t self_offset, const int *fb_count, const int *fb_list, const int32_t *labels,
                         int32_t *idx, double *dist, int32_t *pred, int P, double *part_d, int *part_i,
                         int *part_done);

}  // namespace dsp
