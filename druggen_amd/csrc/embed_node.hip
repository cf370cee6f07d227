// Node embedding of Generator / Discriminator (reference src/model/models.py:52-56, 154-158, applied at :91 / :196):
//     a1 = act(z W1^T + b1) [R,64] ;  a2 = act(a1 W2^T + b2) [R,128]          Linear(E,64) - act - Linear(64,128) - act
// over the R = B N node rows.  On the BLAS + ATen: 4 launches forward, ~8 backward, ~8 in the gradient penalty's second order,
// for 9 k multiply-adds per row.  Two kernels; forward and first backward for all four activations, the second-order form for
// the piecewise-linear ones (ReLU, LeakyReLU(0.01): act'' = 0) only:
//   embed_node_chain   both layers for 32 rows per workgroup.  Forward: activations from the pre-activations.  Second order
//                      (`m1`, `m2` = the forward's a1, a2; `in` = t, the adjoint of the first backward's dz; relu / leaky):
//                      u1 = (t W1^T) . act'(a1), u2 = (u1 W2^T) . act'(a2) -- the adjoints of g2 W2 and of the upstream gradient.
//   embed_node_bwd     g2 = g . act'(a2), g1 = (g2 W2) . act'(a1), dz = g1 W1 (optional).
// The parameter gradients (g2^T a1, g1^T z and their second-order twins g2^T u1, g1^T t) stay dg_linear_wgrad's.
#include "embed_node.h"

namespace dg {
namespace {

constexpr int kH = kNodeH, kC = kNodeC, kEP = 16;      // hidden width, output width, padded input width
constexpr int kRowsN = kNodeRows;
constexpr int kS1 = kH + 1, kS2 = kNodeS2;      // strides of the transposed weights in LDS

template <int ACT, bool MASKED>
__global__ __launch_bounds__(256) void embed_node_chain_kernel(const float* __restrict__ in, const float* __restrict__ m1,
                                                               const float* __restrict__ m2, const float* __restrict__ w1,
                                                               const float* __restrict__ b1, const float* __restrict__ w2,
                                                               const float* __restrict__ b2, float* __restrict__ o1,
                                                               float* __restrict__ o2, int64_t R, int E) {
    __shared__ float w1t[kEP * kS1];            // [e][j]
    __shared__ float w2t[kH * kS2];             // [j][i]
    __shared__ float zs[kRowsN * kEP];
    __shared__ __attribute__((aligned(16))) float a1s[kRowsN * kH];
    const int t = threadIdx.x;
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kRowsN;
    for (int idx = t; idx < kH * kEP; idx += 256) {
        const int j = idx / kEP, e = idx % kEP;
        w1t[e * kS1 + j] = e < E ? w1[j * E + e] : 0.f;
    }
    node_stage_w2t(w2, w2t, t);
    for (int idx = t; idx < kRowsN * kEP; idx += 256) {
        const int64_t r = r0 + idx / kEP;
        const int e = idx % kEP;
        zs[idx] = (r < R && e < E) ? in[r * E + e] : 0.f;
    }
    __syncthreads();
    // layer 1: thread (j = t % 64, row group t / 64) -> rows rg, rg + 4, ...
    {
        const int j = t % kH, rg = t / kH;
        float wj[kEP];
#pragma unroll
        for (int e = 0; e < kEP; ++e) wj[e] = w1t[e * kS1 + j];
        const float bj = (MASKED || !b1) ? 0.f : b1[j];
#pragma unroll
        for (int n = 0; n < kRowsN / 4; ++n) {
            const int row = rg + 4 * n;
            float acc = bj;
#pragma unroll
            for (int e = 0; e < kEP; ++e) acc = fmaf(zs[row * kEP + e], wj[e], acc);
            const int64_t r = r0 + row;
            float a = 0.f;
            if (r < R) {
                a = MASKED ? acc * node_dact<ACT>(m1[r * kH + j]) : node_act<ACT>(acc);
                o1[r * kH + j] = a;
            }
            a1s[row * kH + j] = a;
        }
    }
    __syncthreads();
    node_layer2<ACT, MASKED>(a1s, w2t, b2, m2, o2, r0, R, t);
}

template <int ACT>
__global__ __launch_bounds__(256) void embed_node_bwd_kernel(const float* __restrict__ g, const float* __restrict__ a1,
                                                             const float* __restrict__ a2, const float* __restrict__ w1,
                                                             const float* __restrict__ w2, float* __restrict__ g2o,
                                                             float* __restrict__ g1o, float* __restrict__ dzo, int64_t R, int E) {
    __shared__ __attribute__((aligned(16))) float w2s[kC * kH];              // [i][j] (natural)
    __shared__ float w1s[kH * kEP];             // [j][e]
    __shared__ __attribute__((aligned(16))) float g2s[kRowsN * kC];
    __shared__ __attribute__((aligned(16))) float g1s[kRowsN * kH];
    const int t = threadIdx.x;
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kRowsN;
    for (int idx = t; idx < kH * kEP; idx += 256) {
        const int j = idx / kEP, e = idx % kEP;
        w1s[idx] = e < E ? w1[j * E + e] : 0.f;
    }
    node_bwd_g2_g1<ACT>(g, a1, a2, w2, g2o, g1o, w2s, g2s, g1s, r0, R, t);
    if (!dzo) return;      // (uniform)
    __syncthreads();
    // dz[row][e] = sum_j g1[row][j] w1[j][e]: 32 x 16 (row, e) pairs
#pragma unroll
    for (int n = 0; n < kRowsN * kEP / 256; ++n) {
        const int idx = t + 256 * n;
        const int row = idx / kEP, e = idx % kEP;
        float acc = 0.f;
#pragma unroll 8
        for (int j = 0; j < kH; ++j) acc = fmaf(g1s[row * kH + j], w1s[j * kEP + e], acc);
        const int64_t r = r0 + row;
        if (r < R && e < E) dzo[r * E + e] = acc;
    }
}

}  // namespace
}  // namespace dg

using namespace dg;

/* see include/druggen_hip.h */
extern "C" int dg_embed_node_chain(const float* in, const float* m1, const float* m2, const float* w1, const float* b1,
                                   const float* w2, const float* b2, float* o1, float* o2, int64_t R, int E, int act,
                                   dg_stream_t stream_) {
    if (!in || !w1 || !w2 || !o1 || !o2) return fail(DG_E_ARG, "dg_embed_node_chain: null pointer");
    if ((m1 != nullptr) != (m2 != nullptr))
        return fail(DG_E_ARG, "dg_embed_node_chain: m1 and m2 are given together (second order) or not at all (forward)");
    if (int st = node_check("dg_embed_node_chain", R, E, kEP, act, m1 != nullptr)) return st;
    if (R == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(static_cast<unsigned>((R + kRowsN - 1) / kRowsN));
#define LAUNCH(A, M) hipLaunchKernelGGL((embed_node_chain_kernel<A, M>), grid, dim3(256), 0, stream, in, m1, m2, w1, b1, w2, b2, o1, o2, R, E)
    if (m1) { if (act == kNodeRelu) LAUNCH(kNodeRelu, true); else LAUNCH(kNodeLeaky, true); }
    else if (act == kNodeRelu) LAUNCH(kNodeRelu, false);
    else if (act == kNodeLeaky) LAUNCH(kNodeLeaky, false);
    else if (act == kNodeSigmoid) LAUNCH(kNodeSigmoid, false);
    else LAUNCH(kNodeTanh, false);
#undef LAUNCH
    return check_launch("dg_embed_node_chain");
}

extern "C" int dg_embed_node_bwd(const float* g, const float* a1, const float* a2, const float* w1, const float* w2, float* g2,
                                 float* g1, float* dz, int64_t R, int E, int act, dg_stream_t stream_) {
    if (!g || !a1 || !a2 || !w1 || !w2 || !g2 || !g1) return fail(DG_E_ARG, "dg_embed_node_bwd: null pointer");
    if (int st = node_check("dg_embed_node_bwd", R, E, kEP, act)) return st;
    if (R == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(static_cast<unsigned>((R + kRowsN - 1) / kRowsN));
#define LAUNCH(A) hipLaunchKernelGGL((embed_node_bwd_kernel<A>), grid, dim3(256), 0, stream, g, a1, a2, w1, w2, g2, g1, dz, R, E)
    if (act == kNodeRelu) LAUNCH(kNodeRelu);
    else if (act == kNodeLeaky) LAUNCH(kNodeLeaky);
    else if (act == kNodeSigmoid) LAUNCH(kNodeSigmoid);
    else LAUNCH(kNodeTanh);
#undef LAUNCH
    return check_launch("dg_embed_node_bwd");
}
