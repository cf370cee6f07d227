// Second order of the edge embedding (embed_sym.hip) for the smooth activations, sigmoid and tanh: the backward of
// dg_embed_sym_bwd's input gradient, which the gradient penalty differentiates (reference src/model/loss.py:32-39).
// With act'' != 0 the adjoint t of da reaches every operand of the forward, not only g, W1 and W2.  Per edge row
// (both orientations of a pair are rows; gs = the symmetrised upstream gradient):
//
//     forward         u1 = W1 a + b1,  h1 = f(u1),  u2 = W2 h1 + b2,  y = f(u2)
//     first backward  p2 = gs f'(u2),  dh1 = W2^T p2,  p1 = dh1 f'(u1),  da = W1^T p1
//     s1 = W1 t,  q = s1 f'(u1),  s2 = W2 q,  x = s2 f'(u2)           gg = sym(x)          (dg_embed_sym_bwd2's part)
//     r2 = gs f''(u2) s2                                              the adjoint that reaches u2
//     r1 = f''(u1) s1 dh1 + f'(u1) (W2^T r2)                          the adjoint that reaches u1
//     gW2 = sum p2 q^T + sum r2 h1^T      gb2 = sum r2
//     gW1 = sum p1 t^T + sum r1 a^T       gb1 = sum r1                ga = W1^T r1  (per row)
//
// The tile program of embed_sym_bwd2_kernel with one more [64][128] tile (r2), one more dh_stage and aw2_stage on it, the
// bias sums in the BwdPart slots the piecewise-linear kernel leaves zero, and the per-row input-gradient stage of the
// first backward (on r1 instead of p1).  f' and f'' are taken through the outputs h1 and y that act_fwd gives, as in the
// forward and the first backward.  s1 is recomputed from t where r1 is formed (E <= 16 multiply-adds), never q / f'.
#include "embed_sym.h"

namespace dg {
namespace {

// h1 | p2 | r2 | q | a | t | ij | gs, then x | r1 [64][kD1Pitch] | W1 permuted
constexpr int kSmoothLdsBytes =
    (64 * kHid + 2 * 64 * kC + 64 * kHid + 2 * 64 * kMaxE + kPairs * kC + 64 * kD1Pitch + kHid * 16) * 4 + kPairs * 2 * 4;

// GA: the adjoint of `a` is wanted.  GW: the adjoints of w1, b1, w2, b2 are wanted.  Template parameters, as DA of the first
// backward: a stage behind a run-time test still holds its registers over the whole tile loop.
template <typename T, int EP, int ACT, bool GA, bool GW>
__global__ __launch_bounds__(256) void embed_sym_bwd2_smooth_kernel(
    const float* __restrict__ a, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2p, const float* __restrict__ w2d, const float* __restrict__ b2,
    const T* __restrict__ g, const float* __restrict__ tadj, T* __restrict__ gg, float* __restrict__ ga,
    float* __restrict__ part, int B, int N, int E, int tiles_per_mol) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* h1 = reinterpret_cast<float*>(smem_raw);                 // [64][64] swizzled
    float* d2 = h1 + 64 * kHid;                                      // p2, swizzled [64][128]
    float* r2t = d2 + 64 * kC;                                       // r2, swizzled like p2
    float* hb = r2t + 64 * kC;                                       // q, swizzled like h1
    float(*at)[kMaxE] = reinterpret_cast<float(*)[kMaxE]>(hb + 64 * kHid);
    float(*tt)[kMaxE] = reinterpret_cast<float(*)[kMaxE]>(&at[64][0]);
    int(*ij)[2] = reinterpret_cast<int(*)[2]>(&tt[64][0]);
    float* gst = reinterpret_cast<float*>(&ij[kPairs][0]);           // symmetrised upstream gradient [32][128], then x
    float* d1 = gst + kPairs * kC;                                   // r1 [64][kD1Pitch]
    float4* w1p = reinterpret_cast<float4*>(d1 + 64 * kD1Pitch);     // W1 permuted: w1p[u * 4 + eg] = { W1[u][eg + 4 q] }_q
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (GA) {   // visible after the first barrier of the tile loop
        const int u = threadIdx.x >> 2, eg = threadIdx.x & 3;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = eg + 4 * q < E ? w1[u * E + eg + 4 * q] : 0.f;
        w1p[threadIdx.x] = make_float4(v[0], v[1], v[2], v[3]);
    }
    const int NP = N * (N + 1) / 2;
    const int ut = w & 1, mt = w >> 1;
    f32x16 aw2[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) aw2[0][i] = aw2[1][i] = 0.f;
    float ab2 = 0.f, ab1 = 0.f, aw1[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) aw1[e] = 0.f;
    const int total = B * tiles_per_mol;
    for (int tix = blockIdx.x; tix < total; tix += gridDim.x) {
        const PairTile t{tix / tiles_per_mol, (tix % tiles_per_mol) * kPairs};
        stage_tile<EP, ACT>(a, w1, b1, N, E, NP, t, ij, at, h1);
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        // adjoint rows, in the same (i,j) / (j,i) arrangement as the inputs
        for (int idx = tid; idx < 64 * EP; idx += 256) {
            const int row = idx / EP, e = idx % EP;
            const int pr = row & 31;
            const int i = ij[pr][0], j = ij[pr][1];
            float v = 0.f;
            if (i >= 0 && e < E) v = tadj[tile_edge_row(t.b, N, row, i, j) * E + e];
            tt[row][e] = v;
        }
        __syncthreads();
        {   // q = (W1 t) * f'(u1): thread = (unit u, 16 rows), like layer 1
            const int u = tid & 63, gq = tid >> 6;
            float wv[EP];
#pragma unroll
            for (int e = 0; e < EP; ++e) wv[e] = e < E ? w1[u * E + e] : 0.f;
            for (int r = 0; r < 16; ++r) {
                const int row = gq * 16 + r;
                float sacc = 0.f;
#pragma unroll
                for (int e = 0; e < EP; ++e) sacc = fmaf(wv[e], tt[row][e], sacc);
                const int o = row * kHid + (((u >> 2) ^ (row & 15)) << 2) + (u & 3);
                hb[o] = sacc * act_grad_from_output<ACT>(h1[o]);
            }
        }
        __syncthreads();
        int lo = lane;
        asm volatile("" : "+v"(lo));
        const int half = lo >> 5, col = lo & 31, n = 32 * w + col;
        const float bias2 = b2[n];
        typedef typename raw4<T>::type Raw;
        Raw gr[4][2];
        {   // upstream gradient rows of the 32 pairs, whole rows (see the first backward)
            const int hw = lo >> 5 | (w << 1), l32 = lo & 31;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int pr = hw + 8 * it;
                const int i = ij[pr][0], j = ij[pr][1];
                const int64_t base = static_cast<int64_t>(t.b) * N;
                const int ii = i >= 0 ? i : 0, jj = i >= 0 ? j : 0;       // empty pairs read a valid row, result unused
                gr[it][0] = ld_raw(g + ((base + ii) * N + jj) * kC + 4 * l32);
                gr[it][1] = ld_raw(g + ((base + jj) * N + ii) * kC + 4 * l32);
            }
        }
        f32x16 acc0, acc1, q0, q1;
        {
            const bf16x8* w2f = reinterpret_cast<const bf16x8*>(w2p) + static_cast<size_t>(w) * 4 * 3 * 64 + lo;
            layer2_mfma(h1, w2f, lo, acc0, acc1);   // u2 - b2
            layer2_mfma(hb, w2f, lo, q0, q1);       // s2
        }
        {
            const int hw = lo >> 5 | (w << 1), l32 = lo & 31;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int pr = hw + 8 * it;
                const bool diag = ij[pr][0] == ij[pr][1];
                const float4 v = (diag ? 0.25f : 0.5f) * (cvt_raw(gr[it][0]) + cvt_raw(gr[it][1]));   // diagonal: both blocks carry half
                st4(gst + pr * kC + 4 * l32, ij[pr][0] >= 0 ? v : f4(0.f));
            }
        }
        __syncthreads();
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int pr = (reg & 3) + 8 * (reg >> 2) + 4 * half;
            float p0 = 0.f, p1 = 0.f, r0 = 0.f, r1 = 0.f;
            if (ij[pr][0] >= 0) {   // an empty pair contributes nothing and writes no row
                const float gs = gst[pr * kC + n];   // this (pair, channel) slot belongs to this lane alone: read, then reuse for x
                float f0, c0, f1, c1;
                act_grad2_from_output<ACT>(act_fwd<ACT>(acc0[reg] + bias2), &f0, &c0);
                act_grad2_from_output<ACT>(act_fwd<ACT>(acc1[reg] + bias2), &f1, &c1);
                p0 = gs * f0;
                p1 = gs * f1;
                r0 = gs * c0 * q0[reg];
                r1 = gs * c1 * q1[reg];
                gst[pr * kC + n] = 0.5f * fmaf(q0[reg], f0, q1[reg] * f1);   // explicit: every instance rounds alike
            }
            if (GW) ab2 += r0 + r1;
            if (GA || GW) {
                const int c = n >> 2;
                const int o = pr * kC + (((c & ~15) | ((c & 15) ^ (pr & 15))) << 2) + (n & 3);
                d2[o] = p0;
                d2[32 * kC + o] = p1;
                r2t[o] = r0;
                r2t[32 * kC + o] = r1;
            }
        }
        __syncthreads();
        store_pair_rows(gst, ij, t.b, N, gg, tid);
        if (GA || GW) {
            if (GW) {
                aw2_stage(d2, hb, n, col, half, aw2);    // gW2 += p2^T q
                aw2_stage(r2t, h1, n, col, half, aw2);   //      + r2^T h1
            }
            // (row block mt, unit tile ut): dh1 = p2 W2 and dr = r2 W2
            const bf16x8* w2g = reinterpret_cast<const bf16x8*>(w2d) + static_cast<size_t>(ut) * 8 * 3 * 64 + lo;
            const f32x16 dh = dh_stage(d2, w2g, 32 * mt + col, half);
            const f32x16 dr = dh_stage(r2t, w2g, 32 * mt + col, half);
            const int u = 32 * ut + col;
            float wv[EP];
#pragma unroll
            for (int e = 0; e < EP; ++e) wv[e] = e < E ? w1[u * E + e] : 0.f;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = 32 * mt + (reg & 3) + 8 * (reg >> 2) + 4 * half;
                float fp, fc;
                act_grad2_from_output<ACT>(h1[row * kHid + (((u >> 2) ^ (row & 15)) << 2) + (u & 3)], &fp, &fc);
                float tv[EP];
#pragma unroll
                for (int e4 = 0; e4 < EP; e4 += 4) {       // the row's adjoints as 16-byte LDS reads (broadcast within a half-wave)
                    const float4 t4 = ld4(&tt[row][e4]);
                    tv[e4] = t4.x; tv[e4 + 1] = t4.y; tv[e4 + 2] = t4.z; tv[e4 + 3] = t4.w;
                }
                float s1 = 0.f;   // W1 t again, in the order of the q stage
#pragma unroll
                for (int e = 0; e < EP; ++e) s1 = fmaf(wv[e], tv[e], s1);
                const float p = dh[reg] * fp;
                const float r = fmaf(fp, dr[reg], fc * s1 * dh[reg]);   // explicit: every instance rounds alike
                if (GW) {
                    ab1 += r;
                    float av[EP];
#pragma unroll
                    for (int e4 = 0; e4 < EP; e4 += 4) {
                        const float4 t4 = ld4(&at[row][e4]);
                        av[e4] = t4.x; av[e4 + 1] = t4.y; av[e4 + 2] = t4.z; av[e4 + 3] = t4.w;
                    }
#pragma unroll
                    for (int e = 0; e < EP; ++e) aw1[e] = fmaf(r, av[e], fmaf(p, tv[e], aw1[e]));
                }
                if (GA) d1[row * kD1Pitch + u] = r;
            }
        }
        if (GA) {
            __syncthreads();
            // ga[row][e] = sum_u r1[row][u] W1[u][e]: thread = (tile row, e mod 4); the two halves of a diagonal pair (lanes
            // pr and 32 + pr of the wave) each carry half of the row's r1 and are summed across the wave, as da is
            const int row = lo, eg = w;
            float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
            for (int u4 = 0; u4 < kHid; u4 += 4) {
                const float4 dv = ld4(d1 + row * kD1Pitch + u4);
                const float dvv[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
                for (int uu = 0; uu < 4; ++uu) {
                    const float4 wq = w1p[(u4 + uu) * 4 + eg];
                    s[0] = fmaf(dvv[uu], wq.x, s[0]);
                    s[1] = fmaf(dvv[uu], wq.y, s[1]);
                    s[2] = fmaf(dvv[uu], wq.z, s[2]);
                    s[3] = fmaf(dvv[uu], wq.w, s[3]);
                }
            }
            const int pr = row & 31;
            const int i = ij[pr][0], j = ij[pr][1];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float other = __shfl_xor(s[q], 32, 64);
                const int e = eg + 4 * q;
                if (i < 0 || e >= E || (row >= 32 && i == j)) continue;
                ga[tile_edge_row(t.b, N, row, i, j) * E + e] = i == j ? s[q] + other : s[q];
            }
        }
        __syncthreads();   // LDS tiles are reused by the next iteration
    }
    if (!GW) return;
    // ---- workgroup partials (the layout of the first backward, bias slots included) ----------------
    const int half = lane >> 5, col = lane & 31;
    float* pw = part + static_cast<size_t>(blockIdx.x) * BwdPart::kTotal;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int nn = 32 * w + (reg & 3) + 8 * (reg >> 2) + 4 * half;
            pw[BwdPart::kW2 + nn * kHid + 32 * t2 + col] = aw2[t2][reg];
        }
    // gb2: lanes of the two halves hold the same column
    ab2 += __shfl_xor(ab2, 32, 64);
    if (half == 0) pw[BwdPart::kB2 + 32 * w + col] = ab2;
    // gW1 / gb1: unit u = 32*ut + col is held by 2 half-waves x 2 row blocks (waves ut and ut+2)
    __syncthreads();
    float* red = d2;   // [4 waves][2 halves][32 cols][kMaxE + 1]
    {
        float* slot = red + ((w * 2 + half) * 32 + col) * (kMaxE + 1);
#pragma unroll
        for (int e = 0; e < kMaxE; ++e) slot[e] = e < EP ? aw1[e < EP ? e : 0] : 0.f;
        slot[kMaxE] = ab1;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < kHid * (kMaxE + 1); idx += 256) {
        const int uu = idx / (kMaxE + 1), e = idx % (kMaxE + 1);
        const int utile = uu >> 5, c = uu & 31;
        float s = 0.f;
        for (int mm = 0; mm < 2; ++mm)
            for (int hh = 0; hh < 2; ++hh) s += red[(((utile + 2 * mm) * 2 + hh) * 32 + c) * (kMaxE + 1) + e];
        if (e < kMaxE)
            pw[BwdPart::kW1 + uu * kMaxE + e] = s;
        else
            pw[BwdPart::kB1 + uu] = s;
    }
}

}  // namespace
}  // namespace dg

using namespace dg;

extern "C" int dg_embed_sym_bwd2_smooth(const float* a, const float* w1, const float* b1, const float* w2_packed,
                                        const float* w2_dgrad_packed, const float* b2, const void* g, const float* t,
                                        void* gg, float* ga, float* gw1, float* gb1, float* gw2, float* gb2,
                                        void* workspace, size_t workspace_bytes, int B, int N, int E, int H, int C,
                                        int act, int dtype, dg_stream_t stream_) {
    if (!a || !w1 || !b1 || !w2_packed || !w2_dgrad_packed || !b2 || !g || !t || !gg)
        return fail(DG_E_ARG, "dg_embed_sym_bwd2_smooth: null pointer");
    const int n_w = (gw1 != nullptr) + (gb1 != nullptr) + (gw2 != nullptr) + (gb2 != nullptr);
    if (n_w != 0 && n_w != 4)
        return fail(DG_E_ARG, "dg_embed_sym_bwd2_smooth: gw1, gb1, gw2, gb2 must be all given or all NULL");
    const bool want_w = n_w == 4;
    if (want_w && !workspace) return fail(DG_E_ARG, "dg_embed_sym_bwd2_smooth: null pointer");
    if (!dtype_ok(dtype)) return fail(DG_E_ARG, "dg_embed_sym_bwd2_smooth: unknown dtype %d", dtype);
    if (act != kSigmoid && act != kTanh)
        return fail(DG_E_ARG, "dg_embed_sym_bwd2_smooth: smooth activations only (sigmoid, tanh); relu / leaky: dg_embed_sym_bwd2");
    if (B < 1 || !embed_shape_ok(N, E, H, C, act))
        return fail(DG_E_SHAPE, "dg_embed_sym_bwd2_smooth: unsupported B=%d N=%d E=%d H=%d C=%d act=%d", B, N, E, H, C, act);
    if (want_w && workspace_bytes < dg_embed_sym_workspace_bytes(B, N))
        return fail(DG_E_WORKSPACE, "dg_embed_sym_bwd2_smooth: workspace too small");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int tpm = (N * (N + 1) / 2 + kPairs - 1) / kPairs;
    const int grid = embed_grid(B * tpm, kBwdPerCu);   // fixed by the shape: the partial sums keep their order
    float* part = static_cast<float*>(workspace);
    ProfScope prof(DG_K_EMBED_SYM, stream);
    note_forward(static_cast<int64_t>(B) * N * N);
#define SM_K(T, EP_, ACT_, GA_, GW_)                                                                                   \
    {                                                                                                                  \
        auto kernel = &embed_sym_bwd2_smooth_kernel<T, EP_, ACT_, GA_, GW_>;                                           \
        DG_OPT_IN_LDS(kernel, kSmoothLdsBytes);                                                                        \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), kSmoothLdsBytes, stream, a, w1, b1, w2_packed,               \
                           w2_dgrad_packed, b2, static_cast<const T*>(g), t, static_cast<T*>(gg), ga, part, B, N, E,   \
                           tpm);                                                                                       \
    }
#define SM_O(T, EP_, ACT_)                                                                                             \
    {                                                                                                                  \
        if (ga) { if (want_w) SM_K(T, EP_, ACT_, true, true) else SM_K(T, EP_, ACT_, true, false) }                    \
        else { if (want_w) SM_K(T, EP_, ACT_, false, true) else SM_K(T, EP_, ACT_, false, false) }                     \
    }
#define SM(T, EP_) \
    if (act == kSigmoid) SM_O(T, EP_, kSigmoid) else SM_O(T, EP_, kTanh)
    if (dtype == DG_DTYPE_BF16) {
        if (E <= 8) SM(bf16_t, 8) else SM(bf16_t, 16)
    } else {
        if (E <= 8) SM(float, 8) else SM(float, 16)
    }
#undef SM
#undef SM_O
#undef SM_K
    if (want_w) launch_embed_finish(part, grid, gw1, gb1, gw2, gb2, E, stream);
    return check_launch("dg_embed_sym_bwd2_smooth");
}
