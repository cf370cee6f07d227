// Stages that the node embedding kernels share (embed_node.hip: E <= 16; node_wide.hip: E <= 255): everything behind the
// first Linear is the same Linear(64,128) whatever the input width, so both sets of kernels run the same code there and
// agree bit for bit wherever the first layer does.
#pragma once

#include "common.h"

namespace dg {

constexpr int kNodeH = 64, kNodeC = 128;       // hidden width, output width
constexpr int kNodeRows = 32;                  // rows per workgroup (256 threads)
constexpr int kNodeS2 = kNodeC + 1;            // stride of the transposed W2 in LDS

enum NodeAct { kNodeRelu = 0, kNodeLeaky = 1, kNodeSigmoid = 2, kNodeTanh = 3 };      // the ids of dg_embed_sym_*
template <int ACT>
__device__ __forceinline__ float node_act(float x) {
    switch (ACT) {
        case kNodeRelu: return fmaxf(x, 0.f);
        case kNodeLeaky: return x > 0.f ? x : 0.01f * x;
        case kNodeSigmoid: return 1.0f / (1.0f + __expf(-x));
        default: return tanhf(x);
    }
}
template <int ACT>
__device__ __forceinline__ float node_dact(float a) {      // through the OUTPUT a = act(x)
    switch (ACT) {
        case kNodeRelu: return a > 0.f ? 1.f : 0.f;
        case kNodeLeaky: return a > 0.f ? 1.f : 0.01f;
        case kNodeSigmoid: return a * (1.f - a);
        default: return 1.f - a * a;
    }
}

// w2 [128][64] -> w2t [j][i] (stride kNodeS2)
__device__ __forceinline__ void node_stage_w2t(const float* __restrict__ w2, float* __restrict__ w2t, int t) {
    float4 wv[kNodeC * kNodeH / 1024];      // all eight 16-byte loads of the thread in flight together
#pragma unroll
    for (int n = 0; n < kNodeC * kNodeH / 1024; ++n) wv[n] = ld4(w2 + 4 * (t + 256 * n));
#pragma unroll
    for (int n = 0; n < kNodeC * kNodeH / 1024; ++n) {
        const int idx = 4 * (t + 256 * n);
        const int i = idx / kNodeH, j = idx % kNodeH;
        w2t[j * kNodeS2 + i] = wv[n].x;
        w2t[(j + 1) * kNodeS2 + i] = wv[n].y;
        w2t[(j + 2) * kNodeS2 + i] = wv[n].z;
        w2t[(j + 3) * kNodeS2 + i] = wv[n].w;
    }
}

// layer 2 of the chain over the a1 tile in LDS: thread (i = t % 128, row half t / 128) -> rows rh, rh + 2, ...:
// 16 accumulators, a1 rows as float4 broadcasts
template <int ACT, bool MASKED>
__device__ __forceinline__ void node_layer2(const float* __restrict__ a1s, const float* __restrict__ w2t,
                                            const float* __restrict__ b2, const float* __restrict__ m2,
                                            float* __restrict__ o2, int64_t r0, int64_t R, int t) {
    const int i = t % kNodeC, rh = t / kNodeC;
    float acc[kNodeRows / 2];
    const float bi = (MASKED || !b2) ? 0.f : b2[i];
#pragma unroll
    for (int n = 0; n < kNodeRows / 2; ++n) acc[n] = bi;
#pragma unroll 4
    for (int j = 0; j < kNodeH; j += 4) {
        const float wa = w2t[j * kNodeS2 + i], wb = w2t[(j + 1) * kNodeS2 + i], wc = w2t[(j + 2) * kNodeS2 + i],
                    wd = w2t[(j + 3) * kNodeS2 + i];
#pragma unroll
        for (int n = 0; n < kNodeRows / 2; ++n) {
            const float4 a = *reinterpret_cast<const float4*>(&a1s[(rh + 2 * n) * kNodeH + j]);
            acc[n] = fmaf(a.x, wa, acc[n]);
            acc[n] = fmaf(a.y, wb, acc[n]);
            acc[n] = fmaf(a.z, wc, acc[n]);
            acc[n] = fmaf(a.w, wd, acc[n]);
        }
    }
#pragma unroll
    for (int n = 0; n < kNodeRows / 2; ++n) {
        const int64_t r = r0 + rh + 2 * n;
        if (r < R) o2[r * kNodeC + i] = MASKED ? acc[n] * node_dact<ACT>(m2[r * kNodeC + i]) : node_act<ACT>(acc[n]);
    }
}

// The backward down to g1: g2 = g . act'(a2) (written, and staged in g2s), g1 = (g2 W2) . act'(a1) (written, and left in
// g1s; the caller synchronises before it reads g1s).  w2s [i][j] is W2 as it lies in memory.
template <int ACT>
__device__ __forceinline__ void node_bwd_g2_g1(const float* __restrict__ g, const float* __restrict__ a1,
                                               const float* __restrict__ a2, const float* __restrict__ w2,
                                               float* __restrict__ g2o, float* __restrict__ g1o, float* __restrict__ w2s,
                                               float* __restrict__ g2s, float* __restrict__ g1s, int64_t r0, int64_t R, int t) {
    {
        float4 wv[kNodeC * kNodeH / 1024];
#pragma unroll
        for (int n = 0; n < kNodeC * kNodeH / 1024; ++n) wv[n] = ld4(w2 + 4 * (t + 256 * n));
#pragma unroll
        for (int n = 0; n < kNodeC * kNodeH / 1024; ++n) *reinterpret_cast<float4*>(&w2s[4 * (t + 256 * n)]) = wv[n];
    }
    {
        float4 gv[kNodeRows * kNodeC / 1024], av[kNodeRows * kNodeC / 1024];      // 4 + 4 loads in flight
#pragma unroll
        for (int n = 0; n < kNodeRows * kNodeC / 1024; ++n) {
            const int idx = 4 * (t + 256 * n);
            const int64_t r = r0 + idx / kNodeC;
            gv[n] = r < R ? ld4(g + r * kNodeC + idx % kNodeC) : f4(0.f);
            av[n] = r < R ? ld4(a2 + r * kNodeC + idx % kNodeC) : f4(0.f);
        }
#pragma unroll
        for (int n = 0; n < kNodeRows * kNodeC / 1024; ++n) {
            const int idx = 4 * (t + 256 * n);
            const int64_t r = r0 + idx / kNodeC;
            const float4 v = make_float4(gv[n].x * node_dact<ACT>(av[n].x), gv[n].y * node_dact<ACT>(av[n].y),
                                         gv[n].z * node_dact<ACT>(av[n].z), gv[n].w * node_dact<ACT>(av[n].w));
            if (r < R) st4(g2o + r * kNodeC + idx % kNodeC, v);
            *reinterpret_cast<float4*>(&g2s[idx]) = r < R ? v : f4(0.f);
        }
    }
    __syncthreads();
    // g1[row][j] = (sum_i g2[row][i] w2[i][j]) act'(a1): thread (j = t % 64, row group t / 64), 8 rows each
    const int j = t % kNodeH, rg = t / kNodeH;
    float acc[kNodeRows / 4];
#pragma unroll
    for (int n = 0; n < kNodeRows / 4; ++n) acc[n] = 0.f;
#pragma unroll 4
    for (int i = 0; i < kNodeC; i += 4) {
        const float wa = w2s[i * kNodeH + j], wb = w2s[(i + 1) * kNodeH + j], wc = w2s[(i + 2) * kNodeH + j],
                    wd = w2s[(i + 3) * kNodeH + j];
#pragma unroll
        for (int n = 0; n < kNodeRows / 4; ++n) {
            const float4 v = *reinterpret_cast<const float4*>(&g2s[(rg + 4 * n) * kNodeC + i]);
            acc[n] = fmaf(v.x, wa, acc[n]);
            acc[n] = fmaf(v.y, wb, acc[n]);
            acc[n] = fmaf(v.z, wc, acc[n]);
            acc[n] = fmaf(v.w, wd, acc[n]);
        }
    }
#pragma unroll
    for (int n = 0; n < kNodeRows / 4; ++n) {
        const int row = rg + 4 * n;
        const int64_t r = r0 + row;
        float v = 0.f;
        if (r < R) {
            v = acc[n] * node_dact<ACT>(a1[r * kNodeH + j]);
            g1o[r * kNodeH + j] = v;
        }
        g1s[row * kNodeH + j] = v;
    }
}

// The checks both sets of entries share.  `masked`: the second-order form of the chain, "the same chain with a mask" only
// where act'' = 0.
inline int node_check(const char* who, int64_t R, int E, int emax, int act, bool masked = false) {
    if (R < 0 || E < 1 || E > emax)
        return fail(DG_E_SHAPE, "%s: unsupported shape R=%lld E=%d (1 <= E <= %d)", who, static_cast<long long>(R), E, emax);
    if (act < kNodeRelu || act > kNodeTanh)
        return fail(DG_E_ARG, "%s: activation %d (0 relu, 1 leaky relu 0.01, 2 sigmoid, 3 tanh)", who, act);
    if (masked && act != kNodeRelu && act != kNodeLeaky)
        return fail(DG_E_ARG, "%s: the second-order (masked) form is for relu / leaky relu only, got activation %d", who, act);
    return 0;
}

}  // namespace dg
