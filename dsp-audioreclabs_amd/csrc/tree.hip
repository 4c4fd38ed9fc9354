// tree.hip -- DecisionTreeClassifier.predict / .apply of a fitted single-output tree on gfx950
// (include/dsp_audiorec.h: dsp_tree_predict), the prediction side of the reference's
// TraditionalClassifier('decision_tree') (src/models.py:40-43, :56-58).  Training stays
// scikit-learn's.  A fitted tree is a table of children, feature indices and fp64
// thresholds; scikit-learn casts X to float32 and goes left iff (double)(float)x <= threshold.  The
// walk is comparisons only, so the device's leaf is scikit-learn's with no tolerance.
//
// Two kernels:
//   tree_pack  one 16-byte node {left, right, feature | leaf class, threshold as float32}.  The
//              tested value v is a float32, so v <= t in fp64 is v <= f, f the largest float32 that
//              is <= t: the threshold is rounded DOWN to float32 once here, and the walk compares
//              float32 against float32 -- the same decisions, 16 bytes per node instead of 24.
//   tree_walk  a lane owns a row: it checks that every value of the row stays finite as float32
//              (a NaN is scikit-learn's missing value, the others it refuses: such a row is left to
//              it), then walks.  The node table sits in LDS while it fits (TREE_LDS_NODES), else
//              the 16-byte nodes are read from memory (L2).
// The walk ends on any input: at most max_depth + 1 nodes are visited, and a child index outside
// (node, n_nodes) or a feature index outside [0, D) ends it with -1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsp_audiorec.h"

#pragma clang fp contract(off)

namespace dsp {

static constexpr int TREE_T = 256;             // rows per workgroup (one per lane)
static constexpr int TREE_LDS_NODES = 4096;    // 64 KB of 16-byte nodes
static constexpr size_t TREE_HEAD = 256;       // the counter's slot at the start of the workspace

// the largest float32 that is <= t (t = NaN stays NaN: every comparison with it is false in fp64 too)
__device__ __forceinline__ float float_below(double t)
{
    float f = (float)t;  // to nearest even
    if ((double)f > t) {  // rounded up: one float32 down
        uint32_t b = __float_as_uint(f);
        if (f > 0.0f) b -= 1;
        else if (f < 0.0f) b += 1;
        else b = 0x80000001u;  // t in (-2^-150, 0): below zero, the smallest negative subnormal
        f = __uint_as_float(b);
    }
    return f;
}

__global__ __launch_bounds__(256) void tree_pack(const int32_t *left, const int32_t *right, const int32_t *feature,
                                                 const double *threshold, const int32_t *leaf_class, int n_nodes,
                                                 int4 *nodes, int32_t *unanswered)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    // the walk's count starts at 0 by this kernel's store, not a memset node (as svc_prep's, svm.hip): a
    // captured call is a plain chain of kernels
    if (i == 0) unanswered[0] = 0;
    if (i >= n_nodes) return;
    const int l = left[i];
    int4 n;
    n.x = l;
    n.y = right[i];
    n.z = l == -1 ? leaf_class[i] : feature[i];
    n.w = (int)__float_as_uint(float_below(threshold[i]));
    nodes[i] = n;
}

template <bool LDS>
__global__ __launch_bounds__(TREE_T) void tree_walk(const int4 *__restrict__ nodes, int n_nodes, int D, int max_depth,
                                                    const double *__restrict__ X, int64_t Nq, int32_t *pred,
                                                    int32_t *leaf, int32_t *unanswered)
{
    extern __shared__ __attribute__((aligned(16))) int4 s_nodes[];
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < n_nodes; i += TREE_T) s_nodes[i] = nodes[i];
        __syncthreads();
    }
    const int64_t q = (int64_t)blockIdx.x * TREE_T + threadIdx.x;
    if (q >= Nq) return;
    const double *row = X + q * D;
    bool finite = true;
    for (int d = 0; d < D; d++) finite = finite && (fabsf((float)row[d]) < INFINITY);  // (false for a NaN)
    int at = -1, cls = -1;
    if (finite) {
        int node = 0;
        for (int step = 0; step <= max_depth; step++) {
            const int4 n = LDS ? s_nodes[node] : nodes[node];
            if (n.x == -1) {
                at = node;
                cls = n.z;
                break;
            }
            if ((unsigned)n.z >= (unsigned)D) break;
            const float v = (float)row[n.z];
            const int next = v <= __uint_as_float((uint32_t)n.w) ? n.x : n.y;
            if (next <= node || next >= n_nodes) break;  // a malformed table: no way back, no way out
            node = next;
        }
    }
    pred[q] = cls;
    if (leaf) leaf[q] = at;
    if (at < 0) atomicAdd(unanswered, 1);
}

}  // namespace dsp

extern "C" size_t dsp_tree_workspace_bytes(int64_t n_nodes)
{
    if (n_nodes < 1 || n_nodes > 0x7fffffff) return 0;
    return dsp::TREE_HEAD + (size_t)n_nodes * 16;
}

extern "C" int dsp_tree_lds_nodes(void) { return dsp::TREE_LDS_NODES; }

extern "C" int dsp_tree_predict(const int32_t *children_left, const int32_t *children_right, const int32_t *feature,
                                const double *threshold, const int32_t *leaf_class, int64_t n_nodes, int max_depth,
                                int D, const double *X, int64_t Nq, int32_t *pred, int32_t *leaf, void *workspace,
                                size_t workspace_bytes, void *stream)
{
    if (n_nodes < 1 || n_nodes > 0x7fffffff || max_depth < 0 || D < 1 || D > 4096 || Nq < 0 || !children_left ||
        !children_right || !feature || !threshold || !leaf_class)
        return DSP_ERR_ARGS;
    if (Nq > 0 && (!X || !pred)) return DSP_ERR_ARGS;
    if (!workspace || workspace_bytes < dsp_tree_workspace_bytes(n_nodes)) return DSP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const int64_t blocks = (Nq + dsp::TREE_T - 1) / dsp::TREE_T;
    if (blocks > 0x7fffffff) return DSP_ERR_ARGS;
    const int n = (int)n_nodes;
    int4 *nodes = (int4 *)(ws + dsp::TREE_HEAD);
    // (also for Nq = 0: the count is tree_pack's to clear)
    hipLaunchKernelGGL(dsp::tree_pack, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, s, children_left,
                       children_right, feature, threshold, leaf_class, n, nodes, (int32_t *)ws);
    if (Nq == 0) return hipGetLastError() == hipSuccess ? DSP_OK : DSP_ERR_HIP;
    const dim3 grid((unsigned)blocks), block(dsp::TREE_T);
    if (n <= dsp::TREE_LDS_NODES)
        hipLaunchKernelGGL(dsp::tree_walk<true>, grid, block, (size_t)n * 16, s, nodes, n, D, max_depth, X, Nq, pred,
                           leaf, (int32_t *)ws);
    else
        hipLaunchKernelGGL(dsp::tree_walk<false>, grid, block, 0, s, nodes, n, D, max_depth, X, Nq, pred, leaf,
                           (int32_t *)ws);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSP_OK : DSP_ERR_HIP + (int)e;
}
