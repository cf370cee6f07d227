// Edge embedding on KEPT signs (piecewise-linear activations): dg_embed_sym_fwd_keep stores the sign of every pre-activation
// of both layers, dg_embed_sym_bwd_keep / _bwd2_keep read them where embed_sym.hip's kernels recompute the forward, and
// skip the stages of outputs that are not wanted.  Same tiles, products and summation orders: every output is bit-identical
// to the entries of embed_sym.hip.
#include "embed_sym.h"

namespace dg {
namespace {

// embed_sym_fwd_kernel (embed_sym.hip) that also leaves the signs of both pre-activations (kSignWords words per edge row) for the _keep backward
// kernels.  Layer 2: lanes 0..31 / 32..63 of a wave hold the wave's 32 channels of the rows pr / pr + 4 of one accumulator
// register, so one ballot per register and orientation is word `w` of both rows.  A diagonal pair's row (i,i) sits in both
// orientations with the same values and is written from the first.
template <typename T, int EP, int ACT>
__global__ __launch_bounds__(256, 4) void embed_sym_fwd_keep_kernel(const float* __restrict__ a, const float* __restrict__ w1,
                                                               const float* __restrict__ b1,
                                                               const float* __restrict__ w2p,
                                                               const float* __restrict__ b2, T* __restrict__ out,
                                                               unsigned* __restrict__ signs, int B, int N, int E,
                                                               int tiles_per_mol) {
    __shared__ int ij[kPairs][2];
    __shared__ float at[64][kMaxE];
    __shared__ __attribute__((aligned(16))) float h1[64 * kHid];
    __shared__ __attribute__((aligned(16))) float xt[kPairs * kC];    // symmetrised outputs of the tile
    __shared__ unsigned sg[64 * kSignWords];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, col = lane & 31;
    const int NP = N * (N + 1) / 2;
    const bf16x8* w2f = reinterpret_cast<const bf16x8*>(w2p) + static_cast<size_t>(w) * 4 * 3 * 64 + lane;
    const int n = 32 * w + col;
    const float bias2 = b2[n];
    const int total = B * tiles_per_mol;
    for (int tix = blockIdx.x; tix < total; tix += gridDim.x) {
        const PairTile t{tix / tiles_per_mol, (tix % tiles_per_mol) * kPairs};
        stage_tile<EP, ACT, true>(a, w1, b1, N, E, NP, t, ij, at, h1, sg);
        f32x16 acc0, acc1;
        layer2_mfma(h1, w2f, lane, acc0, acc1);
        unsigned k0 = 0u, k1 = 0u;   // lane `reg` of each half keeps the words of register `reg`: one LDS store per orientation
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int pr = (reg & 3) + 8 * (reg >> 2) + 4 * half;
            const float v0 = acc0[reg] + bias2, v1 = acc1[reg] + bias2;
            xt[pr * kC + n] = 0.5f * (act_fwd<ACT>(v0) + act_fwd<ACT>(v1));
            const unsigned long long m0 = __builtin_amdgcn_ballot_w64(v0 > 0.f), m1 = __builtin_amdgcn_ballot_w64(v1 > 0.f);
            if (col == reg) {
                k0 = static_cast<unsigned>(half ? m0 >> 32 : m0);
                k1 = static_cast<unsigned>(half ? m1 >> 32 : m1);
            }
        }
        if (col < 16) {
            const int pr = (col & 3) + 8 * (col >> 2) + 4 * half;
            sg[pr * kSignWords + w] = k0;
            sg[(32 + pr) * kSignWords + w] = k1;
        }
        __syncthreads();
        store_pair_rows(xt, ij, t.b, N, out, static_cast<int>(threadIdx.x));
        for (int idx = threadIdx.x; idx < 64 * kSignWords; idx += 256) {
            const int row = idx / kSignWords, k = idx % kSignWords;
            const int i = ij[row & 31][0], j = ij[row & 31][1];
            if (i < 0 || (row >= 32 && i == j)) continue;
            signs[tile_edge_row(t.b, N, row, i, j) * kSignWords + k] = sg[idx];
        }
        __syncthreads();   // LDS tiles are reused by the next iteration
    }
}

// ------------------------------------------------- backward kernels on the forward's signs ----
// dg_embed_sym_fwd_keep left the sign of every pre-activation (kSignWords words per edge row), so nothing of the forward is
// recomputed for its ReLU masks: dpre2 = gs * act'(sign), dpre1 = dh1 * act'(sign).  The wanted outputs are template
// parameters (see DA of embed_sym_bwd_kernel).  W (weight gradients): layer 1 is still recomputed from `a` by stage_tile -- dW2 needs the VALUES
// of h1 -- and the stages, products, accumulation and partial-sum orders are those of embed_sym_bwd_kernel, bit for bit.
// Without W the tile program is: gradient rows -> symmetrise -> dpre2 -> dh = dpre2 W2 -> dpre1 -> da; no gather of `a`, no
// h1 tile, no partial sums: 52 KB of LDS (E <= 8) instead of 71, five barriers per tile instead of seven.
template <int ACT>
__device__ __forceinline__ float act_grad_from_sign(unsigned bit) {
    return bit ? 1.f : (ACT == kRelu ? 0.f : 0.01f);
}

// the pair table alone (first step of stage_tile)
__device__ __forceinline__ void stage_pairs(int N, int NP, PairTile t, int (*ij)[2], int tid) {
    if (tid < kPairs) {
        const int p = t.p0 + tid;
        int i = 0, j = 0;
        if (p < NP) pair_to_ij(p, N, &i, &j);
        ij[tid][0] = p < NP ? i : -1;
        ij[tid][1] = j;
    }
    __syncthreads();
}
// sign words of the tile's 64 rows -> LDS (rows of empty pairs: zero, their results are never used)
__device__ __forceinline__ void stage_signs(const unsigned* __restrict__ signs, int N, PairTile t, const int (*ij)[2],
                                            unsigned* sg, int tid) {
    for (int idx = tid; idx < 64 * kSignWords; idx += 256) {
        const int row = idx / kSignWords, k = idx % kSignWords;
        const int i = ij[row & 31][0], j = ij[row & 31][1];
        sg[idx] = i >= 0 ? signs[tile_edge_row(t.b, N, row, i, j) * kSignWords + k] : 0u;
    }
}
// upstream gradient rows (b,i,j) and (b,j,i) of the tile's 32 pairs: whole rows, one half-wave per row (see embed_sym_bwd_kernel)
template <typename T>
__device__ __forceinline__ void load_grad_rows(const T* __restrict__ g, const int (*ij)[2], int b, int N, int lo, int w,
                                               typename raw4<T>::type (&gr)[4][2]) {
    const int hw = lo >> 5 | (w << 1), l32 = lo & 31;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int pr = hw + 8 * it;
        const int i = ij[pr][0], j = ij[pr][1];
        const int64_t base = static_cast<int64_t>(b) * N;
        const int ii = i >= 0 ? i : 0, jj = i >= 0 ? j : 0;       // empty pairs read a valid row, result unused
        gr[it][0] = ld_raw(g + ((base + ii) * N + jj) * kC + 4 * l32);
        gr[it][1] = ld_raw(g + ((base + jj) * N + ii) * kC + 4 * l32);
    }
}
template <typename Raw>
__device__ __forceinline__ void sym_grad_rows(const Raw (&gr)[4][2], const int (*ij)[2], float* gst, int lo, int w) {
    const int hw = lo >> 5 | (w << 1), l32 = lo & 31;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int pr = hw + 8 * it;
        const bool diag = ij[pr][0] == ij[pr][1];
        const float4 v = (diag ? 0.25f : 0.5f) * (cvt_raw(gr[it][0]) + cvt_raw(gr[it][1]));   // diagonal: both blocks carry half
        st4(gst + pr * kC + 4 * l32, ij[pr][0] >= 0 ? v : f4(0.f));
    }
}
// offset of (row, unit u) in an XOR-swizzled [64][kHid] tile
__device__ __forceinline__ int hid_off(int row, int u) { return row * kHid + (((u >> 2) ^ (row & 15)) << 2) + (u & 3); }
// offset of (row, channel n) in the swizzled [64][kC] dpre2 tile
__device__ __forceinline__ int d2_off(int row, int n) {
    const int c = n >> 2;
    return row * kC + (((c & ~15) | ((c & 15) ^ (row & 15))) << 2) + (n & 3);
}

constexpr int bwd_keep_lds_bytes(int EP, bool W) {
    return (64 * kC + 64 * kHid + kHid * EP + (W ? 64 * kHid + 64 * kMaxE : 0)) * 4 + kPairs * 2 * 4 + 64 * kSignWords * 4;
}

template <typename T, int EP, int ACT, bool DA, bool W>
__global__ __launch_bounds__(256, W ? 2 : 3) void embed_sym_bwd_keep_kernel(
    const float* __restrict__ a, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2d, const T* __restrict__ g, const unsigned* __restrict__ signs, float* __restrict__ da,
    float* __restrict__ part, int B, int N, int E, int tiles_per_mol) {
    constexpr int Q = EP / 4;                                        // input features per (unit, e mod 4) in the da stage
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* d2 = reinterpret_cast<float*>(smem_raw);                 // dpre2, swizzled [64][128]
    float* d1 = d2 + 64 * kC;                                        // dpre1, swizzled [64][64]
    float* gst = d1;   // symmetrised upstream gradient of the tile [32 pairs][128]: dead before d1 is written
    int(*ij)[2] = reinterpret_cast<int(*)[2]>(d1 + 64 * kHid);
    unsigned* sg = reinterpret_cast<unsigned*>(&ij[kPairs][0]);      // [64][kSignWords]
    float* w1p = reinterpret_cast<float*>(sg + 64 * kSignWords);     // W1 permuted: w1p[(u * 4 + eg) * Q + q] = W1[u][eg + 4 q]
    float* h1 = w1p + kHid * EP;                                     // W only: [64][64] swizzled
    float(*at)[kMaxE] = reinterpret_cast<float(*)[kMaxE]>(h1 + 64 * kHid);   // W only
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (DA) {   // visible after the first barrier of the tile loop
        const int u = tid >> 2, eg = tid & 3;
#pragma unroll
        for (int q = 0; q < Q; ++q) w1p[tid * Q + q] = eg + 4 * q < E ? w1[u * E + eg + 4 * q] : 0.f;
    }
    const int NP = N * (N + 1) / 2;
    const int ut = w & 1, mt = w >> 1;   // dgrad: output tile ut (32 hidden units), row block mt
    f32x16 aw2[2];                       // dW2 tiles (n tile w) x (unit tile 0,1)
#pragma unroll
    for (int i = 0; i < 16; ++i) aw2[0][i] = aw2[1][i] = 0.f;
    float ab2 = 0.f, ab1 = 0.f, aw1[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) aw1[e] = 0.f;
    const int total = B * tiles_per_mol;
    for (int tix = blockIdx.x; tix < total; tix += gridDim.x) {
        const PairTile t{tix / tiles_per_mol, (tix % tiles_per_mol) * kPairs};
        if (W)
            stage_tile<EP, ACT>(a, w1, b1, N, E, NP, t, ij, at, h1);
        else
            stage_pairs(N, NP, t, ij, tid);
        int lo = lane;   // per-iteration opaque copy of the lane id (see embed_sym_bwd_kernel)
        asm volatile("" : "+v"(lo));
        const int half = lo >> 5, col = lo & 31, n = 32 * w + col;
        typename raw4<T>::type gr[4][2];
        load_grad_rows(g, ij, t.b, N, lo, w, gr);
        stage_signs(signs, N, t, ij, sg, lo + 64 * w);
        sym_grad_rows(gr, ij, gst, lo, w);
        __syncthreads();
        // dpre2 in the accumulator layout -> LDS (swizzled like a row-GEMM A tile)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int pr = (reg & 3) + 8 * (reg >> 2) + 4 * half;
            float p0 = 0.f, p1 = 0.f;
            if (ij[pr][0] >= 0) {
                const float gs = gst[pr * kC + n];
                p0 = gs * act_grad_from_sign<ACT>(sg[pr * kSignWords + w] >> col & 1u);
                p1 = gs * act_grad_from_sign<ACT>(sg[(32 + pr) * kSignWords + w] >> col & 1u);
            }
            if (W) ab2 += p0 + p1;
            d2[d2_off(pr, n)] = p0;
            d2[d2_off(32 + pr, n)] = p1;
        }
        __syncthreads();
        if (W) aw2_stage(d2, h1, n, col, half, aw2);   // dW2 += dpre2^T h1
        // dh1 = dpre2 W2 for (row block mt, unit tile ut); dpre1 = dh1 * act'(sign)
        const f32x16 dh = dh_stage(d2, reinterpret_cast<const bf16x8*>(w2d) + static_cast<size_t>(ut) * 8 * 3 * 64 + lo, 32 * mt + col, half);
        const int u = 32 * ut + col;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = 32 * mt + (reg & 3) + 8 * (reg >> 2) + 4 * half;
            const float p = dh[reg] * act_grad_from_sign<ACT>(sg[row * kSignWords + 4 + ut] >> col & 1u);
            if (W) {
                ab1 += p;
                float av[EP];
#pragma unroll
                for (int e4 = 0; e4 < EP; e4 += 4) {       // the row's inputs as 16-byte LDS reads (broadcast within a half-wave)
                    const float4 t4 = ld4(&at[row][e4]);
                    av[e4] = t4.x; av[e4 + 1] = t4.y; av[e4 + 2] = t4.z; av[e4 + 3] = t4.w;
                }
#pragma unroll
                for (int e = 0; e < EP; ++e) aw1[e] = fmaf(p, av[e], aw1[e]);
            }
            if (DA) d1[hid_off(row, u)] = p;
        }
        if (DA) {
            __syncthreads();
            // da[row][e] = sum_u dpre1[row][u] W1[u][e]: thread = (tile row, e mod 4); the two halves of a diagonal pair
            // (rows pr and 32 + pr = lanes pr and 32 + pr of the wave) are summed across the wave
            const int row = lo, eg = w;
            float s[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) s[q] = 0.f;
#pragma unroll 4
            for (int u4 = 0; u4 < kHid; u4 += 4) {
                const float4 dv = ld4(d1 + hid_off(row, u4));
                const float dvv[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
                for (int uu = 0; uu < 4; ++uu) {
                    const float* wv = w1p + ((u4 + uu) * 4 + eg) * Q;   // one broadcast 8- / 16-byte read
#pragma unroll
                    for (int q = 0; q < Q; ++q) s[q] = fmaf(dvv[uu], wv[q], s[q]);
                }
            }
            const int pr = row & 31;
            const int i = ij[pr][0], j = ij[pr][1];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float other = __shfl_xor(s[q], 32, 64);
                const int e = eg + 4 * q;
                if (i < 0 || e >= E || (row >= 32 && i == j)) continue;
                da[tile_edge_row(t.b, N, row, i, j) * E + e] = i == j ? s[q] + other : s[q];
            }
        }
        __syncthreads();
    }
    if (!W) return;
    // ---- workgroup partials (layout and summation order of embed_sym_bwd_kernel) ------------------
    const int half = lane >> 5, col = lane & 31, n = 32 * w + col;
    float* pw = part + static_cast<size_t>(blockIdx.x) * BwdPart::kTotal;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int nn = 32 * w + (reg & 3) + 8 * (reg >> 2) + 4 * half;
            pw[BwdPart::kW2 + nn * kHid + 32 * t2 + col] = aw2[t2][reg];
        }
    ab2 += __shfl_xor(ab2, 32, 64);
    if (half == 0) pw[BwdPart::kB2 + n] = ab2;
    __syncthreads();
    float* red = d2;   // [4 waves][2 halves][32 cols][kMaxE + 1]
    {
        float* slot = red + ((w * 2 + half) * 32 + col) * (kMaxE + 1);
#pragma unroll
        for (int e = 0; e < kMaxE; ++e) slot[e] = e < EP ? aw1[e < EP ? e : 0] : 0.f;
        slot[kMaxE] = ab1;
    }
    __syncthreads();
    for (int idx = tid; idx < kHid * (kMaxE + 1); idx += 256) {
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

// Second order on the forward's signs (see embed_sym_bwd2_kernel): both activations' derivatives are sign bits, so neither
// layer of the forward is recomputed and `a` is not read.  Without W (gw1, gw2 not wanted) only x = (W2 q) * act'(f) is left:
// the upstream gradient g is not read either.
constexpr int bwd2_keep_lds_bytes(bool W) {
    return (64 * kHid + 64 * kMaxE + kPairs * kC + (W ? 64 * kC : 0)) * 4 + kPairs * 2 * 4 + 64 * kSignWords * 4;
}

template <typename T, int EP, int ACT, bool W>
__global__ __launch_bounds__(256, W ? 2 : 3) void embed_sym_bwd2_keep_kernel(
    const float* __restrict__ w1, const float* __restrict__ w2p, const float* __restrict__ w2d, const T* __restrict__ g,
    const float* __restrict__ tadj, const unsigned* __restrict__ signs, T* __restrict__ gg, float* __restrict__ part,
    int B, int N, int E, int tiles_per_mol) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* hb = reinterpret_cast<float*>(smem_raw);                 // q, swizzled [64][64]
    float* gst = hb + 64 * kHid;                                     // symmetrised upstream gradient [32][128], then x
    float(*tt)[kMaxE] = reinterpret_cast<float(*)[kMaxE]>(gst + kPairs * kC);
    int(*ij)[2] = reinterpret_cast<int(*)[2]>(&tt[64][0]);
    unsigned* sg = reinterpret_cast<unsigned*>(&ij[kPairs][0]);      // [64][kSignWords]
    float* d2 = reinterpret_cast<float*>(sg + 64 * kSignWords);      // W only: p2, swizzled [64][128]
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int NP = N * (N + 1) / 2;
    const int ut = w & 1, mt = w >> 1;
    f32x16 aw2[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) aw2[0][i] = aw2[1][i] = 0.f;
    float aw1[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) aw1[e] = 0.f;
    const int total = B * tiles_per_mol;
    for (int tix = blockIdx.x; tix < total; tix += gridDim.x) {
        const PairTile t{tix / tiles_per_mol, (tix % tiles_per_mol) * kPairs};
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        stage_pairs(N, NP, t, ij, tid);
        // adjoint rows, in the (i,j) / (j,i) arrangement of the tile
        for (int idx = tid; idx < 64 * EP; idx += 256) {
            const int row = idx / EP, e = idx % EP;
            const int i = ij[row & 31][0], j = ij[row & 31][1];
            float v = 0.f;
            if (i >= 0 && e < E) v = tadj[tile_edge_row(t.b, N, row, i, j) * E + e];
            tt[row][e] = v;
        }
        stage_signs(signs, N, t, ij, sg, tid);
        __syncthreads();
        {   // q = (W1 t) * act'(layer-1 sign): thread = (unit u, 16 rows), like layer 1
            const int u = tid & 63, gq = tid >> 6;
            float wv[EP];
#pragma unroll
            for (int e = 0; e < EP; ++e) wv[e] = e < E ? w1[u * E + e] : 0.f;
            for (int r = 0; r < 16; ++r) {
                const int row = gq * 16 + r;
                float sacc = 0.f;
#pragma unroll
                for (int e = 0; e < EP; ++e) sacc = fmaf(wv[e], tt[row][e], sacc);
                hb[hid_off(row, u)] = sacc * act_grad_from_sign<ACT>(sg[row * kSignWords + 4 + (u >> 5)] >> (u & 31) & 1u);
            }
        }
        __syncthreads();
        int lo = lane;
        asm volatile("" : "+v"(lo));
        const int half = lo >> 5, col = lo & 31, n = 32 * w + col;
        typename raw4<T>::type gr[4][2];
        if (W) load_grad_rows(g, ij, t.b, N, lo, w, gr);
        f32x16 q0, q1;
        layer2_mfma(hb, reinterpret_cast<const bf16x8*>(w2p) + static_cast<size_t>(w) * 4 * 3 * 64 + lo, lo, q0, q1);
        if (W) {
            sym_grad_rows(gr, ij, gst, lo, w);
            __syncthreads();
        }
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int pr = (reg & 3) + 8 * (reg >> 2) + 4 * half;
            float p0 = 0.f, p1 = 0.f;
            if (ij[pr][0] >= 0) {
                const float d0 = act_grad_from_sign<ACT>(sg[pr * kSignWords + w] >> col & 1u);
                const float d1v = act_grad_from_sign<ACT>(sg[(32 + pr) * kSignWords + w] >> col & 1u);
                if (W) {
                    const float gs = gst[pr * kC + n];   // this (pair, channel) slot belongs to this lane alone: read, then reuse for x
                    p0 = gs * d0;
                    p1 = gs * d1v;
                }
                gst[pr * kC + n] = 0.5f * (q0[reg] * d0 + q1[reg] * d1v);
            }
            if (W) {
                d2[d2_off(pr, n)] = p0;
                d2[d2_off(32 + pr, n)] = p1;
            }
        }
        __syncthreads();
        store_pair_rows(gst, ij, t.b, N, gg, tid);
        if (W) {
            // gW2 += p2^T q : contraction over the 64 tile rows
            aw2_stage(d2, hb, n, col, half, aw2);
            // dh1 = p2 W2 for (row block mt, unit tile ut); p1 = dh1 * act'(sign); gW1 += p1^T t
            const f32x16 dh = dh_stage(d2, reinterpret_cast<const bf16x8*>(w2d) + static_cast<size_t>(ut) * 8 * 3 * 64 + lo, 32 * mt + col, half);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = 32 * mt + (reg & 3) + 8 * (reg >> 2) + 4 * half;
                const float p = dh[reg] * act_grad_from_sign<ACT>(sg[row * kSignWords + 4 + ut] >> col & 1u);
                float av[EP];
#pragma unroll
                for (int e4 = 0; e4 < EP; e4 += 4) {
                    const float4 t4 = ld4(&tt[row][e4]);
                    av[e4] = t4.x; av[e4 + 1] = t4.y; av[e4 + 2] = t4.z; av[e4 + 3] = t4.w;
                }
#pragma unroll
                for (int e = 0; e < EP; ++e) aw1[e] = fmaf(p, av[e], aw1[e]);
            }
        }
        __syncthreads();
    }
    if (!W) return;
    // ---- workgroup partials (layout and summation order of embed_sym_bwd2_kernel; the bias slots stay zero) ------------
    const int half = lane >> 5, col = lane & 31;
    float* pw = part + static_cast<size_t>(blockIdx.x) * BwdPart::kTotal;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int nn = 32 * w + (reg & 3) + 8 * (reg >> 2) + 4 * half;
            pw[BwdPart::kW2 + nn * kHid + 32 * t2 + col] = aw2[t2][reg];
        }
    __syncthreads();
    float* red = d2;   // [4 waves][2 halves][32 cols][kMaxE]
    {
        float* slot = red + ((w * 2 + half) * 32 + col) * kMaxE;
#pragma unroll
        for (int e = 0; e < kMaxE; ++e) slot[e] = e < EP ? aw1[e < EP ? e : 0] : 0.f;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < kHid * kMaxE; idx += 256) {
        const int uu = idx / kMaxE, e = idx % kMaxE;
        const int utile = uu >> 5, c = uu & 31;
        float sum = 0.f;
        for (int mm = 0; mm < 2; ++mm)
            for (int hh = 0; hh < 2; ++hh) sum += red[(((utile + 2 * mm) * 2 + hh) * 32 + c) * kMaxE + e];
        pw[BwdPart::kW1 + uu * kMaxE + e] = sum;
    }
}

// Workgroups of a _keep backward instance that one CU holds (256 threads, `lds` bytes of dynamic LDS): asked once per instance,
// it sizes the grid of the instances without weight gradients (52 KB of LDS for E <= 8: three per CU where 160 KB allow it).
template <typename K>
int resident_per_cu(K kernel, int lds, std::atomic<int>* cache) {
    int v = cache->load(std::memory_order_relaxed);
    if (v == 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, 256, lds) != hipSuccess) {
            (void)hipGetLastError();
            nb = kBwdPerCu;
        }
        v = nb < 1 ? 1 : (nb > 4 ? 4 : nb);
        cache->store(v, std::memory_order_relaxed);
    }
    return v;
}

}  // namespace
}  // namespace dg

using namespace dg;

// ---- the same three entries on kept signs (piecewise-linear activations) ----------------------------------------------
extern "C" size_t dg_embed_sym_sign_words(int B, int N) {
    return B < 0 || N < 0 ? 0 : static_cast<size_t>(B) * N * N * kSignWords;
}

extern "C" int dg_embed_sym_fwd_keep(const float* a, const float* w1, const float* b1, const float* w2_packed,
                                     const float* b2, void* out, uint32_t* signs, int B, int N, int E, int H, int C,
                                     int act, int dtype, dg_stream_t stream_) {
    if (!a || !w1 || !b1 || !w2_packed || !b2 || !out || !signs) return fail(DG_E_ARG, "dg_embed_sym_fwd_keep: null pointer");
    if (!dtype_ok(dtype)) return fail(DG_E_ARG, "dg_embed_sym_fwd_keep: unknown dtype %d", dtype);
    if (act != kRelu && act != kLeaky)
        return fail(DG_E_ARG, "dg_embed_sym_fwd_keep: only piecewise-linear activations (relu, leaky) are described by their signs");
    if (B < 0 || !embed_shape_ok(N, E, H, C, act))
        return fail(DG_E_SHAPE, "dg_embed_sym_fwd_keep: unsupported N=%d E=%d H=%d C=%d act=%d (need E<=16, H=64, C=128)", N,
                    E, H, C, act);
    if (B == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int tpm = (N * (N + 1) / 2 + kPairs - 1) / kPairs;
    ProfScope prof(DG_K_EMBED_SYM, stream);
    note_forward(static_cast<int64_t>(B) * N * N);
#define FWD_A(T, EP_, ACT_)                                                                                           \
    hipLaunchKernelGGL((embed_sym_fwd_keep_kernel<T, EP_, ACT_>), dim3(embed_grid(B * tpm, 8)), dim3(256), 0, stream, a, \
                       w1, b1, w2_packed, b2, static_cast<T*>(out), signs, B, N, E, tpm);
#define FWD(T, EP_) \
    if (act == kRelu) { FWD_A(T, EP_, kRelu) } else { FWD_A(T, EP_, kLeaky) }
    if (dtype == DG_DTYPE_BF16) {
        if (E <= 8) { FWD(bf16_t, 8) } else { FWD(bf16_t, 16) }
    } else {
        if (E <= 8) { FWD(float, 8) } else { FWD(float, 16) }
    }
#undef FWD_A
#undef FWD
    return check_launch("dg_embed_sym_fwd_keep");
}

extern "C" int dg_embed_sym_bwd_keep(const float* a, const float* w1, const float* b1, const float* w2_packed,
                                     const float* w2_dgrad_packed, const float* b2, const void* g, const uint32_t* signs,
                                     float* da, float* dw1, float* db1, float* dw2, float* db2, void* workspace,
                                     size_t workspace_bytes, int B, int N, int E, int H, int C, int act, int dtype,
                                     dg_stream_t stream_) {
    if (!a || !w1 || !b1 || !w2_packed || !w2_dgrad_packed || !b2 || !g || !signs)
        return fail(DG_E_ARG, "dg_embed_sym_bwd_keep: null pointer");
    const int n_w = (dw1 != nullptr) + (db1 != nullptr) + (dw2 != nullptr) + (db2 != nullptr);
    if (n_w != 0 && n_w != 4)
        return fail(DG_E_ARG, "dg_embed_sym_bwd_keep: dw1, db1, dw2, db2 must be all given or all NULL");
    const bool want_w = n_w == 4;
    if (want_w && !workspace) return fail(DG_E_ARG, "dg_embed_sym_bwd_keep: null pointer");
    if (!dtype_ok(dtype)) return fail(DG_E_ARG, "dg_embed_sym_bwd_keep: unknown dtype %d", dtype);
    if (act != kRelu && act != kLeaky)
        return fail(DG_E_ARG, "dg_embed_sym_bwd_keep: only piecewise-linear activations (relu, leaky) are described by their signs");
    if (B < 1 || !embed_shape_ok(N, E, H, C, act))
        return fail(DG_E_SHAPE, "dg_embed_sym_bwd_keep: unsupported B=%d N=%d E=%d H=%d C=%d act=%d", B, N, E, H, C, act);
    if (want_w && workspace_bytes < dg_embed_sym_workspace_bytes(B, N))
        return fail(DG_E_WORKSPACE, "dg_embed_sym_bwd_keep: workspace too small");
    if (!da && !want_w) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int tpm = (N * (N + 1) / 2 + kPairs - 1) / kPairs;
    const int grid_w = embed_grid(B * tpm, kBwdPerCu);   // the grid of dg_embed_sym_bwd: the partial sums keep their order
    float* part = static_cast<float*>(workspace);
    ProfScope prof(DG_K_EMBED_SYM, stream);
    note_forward(static_cast<int64_t>(B) * N * N);
#define BWD_D(T, EP_, ACT_, DA_, W_)                                                                                 \
    {                                                                                                                \
        constexpr int lds_bytes = bwd_keep_lds_bytes(EP_, W_);                                                       \
        auto kernel = &embed_sym_bwd_keep_kernel<T, EP_, ACT_, DA_, W_>;                                             \
        DG_OPT_IN_LDS(kernel, lds_bytes);                                                                            \
        static std::atomic<int> per_cu_{0};                                                                          \
        const int grid = W_ ? grid_w : embed_grid(B * tpm, resident_per_cu(kernel, lds_bytes, &per_cu_));            \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds_bytes, stream, a, w1, b1, w2_dgrad_packed,             \
                           static_cast<const T*>(g), signs, da, part, B, N, E, tpm);                                 \
    }
#define BWD_A(T, EP_, ACT_)                                                                                          \
    {                                                                                                                \
        if (!want_w) BWD_D(T, EP_, ACT_, true, false) else if (da) BWD_D(T, EP_, ACT_, true, true)                   \
        else BWD_D(T, EP_, ACT_, false, true)                                                                        \
    }
#define BWD(T, EP_) \
    if (act == kRelu) BWD_A(T, EP_, kRelu) else BWD_A(T, EP_, kLeaky)
    if (dtype == DG_DTYPE_BF16) {
        if (E <= 8) BWD(bf16_t, 8) else BWD(bf16_t, 16)
    } else {
        if (E <= 8) BWD(float, 8) else BWD(float, 16)
    }
#undef BWD_A
#undef BWD_D
#undef BWD
    if (want_w)
        launch_embed_finish(part, grid_w, dw1, db1, dw2, db2, E, stream);
    return check_launch("dg_embed_sym_bwd_keep");
}

extern "C" int dg_embed_sym_bwd2_keep(const float* a, const float* w1, const float* b1, const float* w2_packed,
                                      const float* w2_dgrad_packed, const float* b2, const void* g, const float* t,
                                      const uint32_t* signs, void* gg, float* gw1, float* gw2, void* workspace,
                                      size_t workspace_bytes, int B, int N, int E, int H, int C, int act, int dtype,
                                      dg_stream_t stream_) {
    if (!a || !w1 || !b1 || !w2_packed || !w2_dgrad_packed || !b2 || !g || !t || !signs || !gg)
        return fail(DG_E_ARG, "dg_embed_sym_bwd2_keep: null pointer");
    if ((gw1 != nullptr) != (gw2 != nullptr))
        return fail(DG_E_ARG, "dg_embed_sym_bwd2_keep: gw1, gw2 must be both given or both NULL");
    const bool want_w = gw1 != nullptr;
    if (want_w && !workspace) return fail(DG_E_ARG, "dg_embed_sym_bwd2_keep: null pointer");
    if (!dtype_ok(dtype)) return fail(DG_E_ARG, "dg_embed_sym_bwd2_keep: unknown dtype %d", dtype);
    if (act != kRelu && act != kLeaky)
        return fail(DG_E_ARG, "dg_embed_sym_bwd2_keep: only piecewise-linear activations (relu, leaky) have this closed form");
    if (B < 1 || !embed_shape_ok(N, E, H, C, act))
        return fail(DG_E_SHAPE, "dg_embed_sym_bwd2_keep: unsupported B=%d N=%d E=%d H=%d C=%d act=%d", B, N, E, H, C, act);
    if (want_w && workspace_bytes < dg_embed_sym_workspace_bytes(B, N))
        return fail(DG_E_WORKSPACE, "dg_embed_sym_bwd2_keep: workspace too small");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int tpm = (N * (N + 1) / 2 + kPairs - 1) / kPairs;
    const int grid_w = embed_grid(B * tpm, kBwdPerCu);   // the grid of dg_embed_sym_bwd2: the partial sums keep their order
    float* part = static_cast<float*>(workspace);
    ProfScope prof(DG_K_EMBED_SYM, stream);
    note_forward(static_cast<int64_t>(B) * N * N);
#define BWD2_W(T, EP_, ACT_, W_)                                                                                      \
    {                                                                                                                 \
        constexpr int lds_bytes = bwd2_keep_lds_bytes(W_);                                                            \
        auto kernel = &embed_sym_bwd2_keep_kernel<T, EP_, ACT_, W_>;                                                  \
        DG_OPT_IN_LDS(kernel, lds_bytes);                                                                             \
        static std::atomic<int> per_cu_{0};                                                                           \
        const int grid = W_ ? grid_w : embed_grid(B * tpm, resident_per_cu(kernel, lds_bytes, &per_cu_));             \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds_bytes, stream, w1, w2_packed, w2_dgrad_packed,          \
                           static_cast<const T*>(g), t, signs, static_cast<T*>(gg), part, B, N, E, tpm);              \
    }
#define BWD2_A(T, EP_, ACT_) \
    { if (want_w) BWD2_W(T, EP_, ACT_, true) else BWD2_W(T, EP_, ACT_, false) }
#define BWD2(T, EP_) \
    if (act == kRelu) BWD2_A(T, EP_, kRelu) else BWD2_A(T, EP_, kLeaky)
    if (dtype == DG_DTYPE_BF16) {
        if (E <= 8) BWD2(bf16_t, 8) else BWD2(bf16_t, 16)
    } else {
        if (E <= 8) BWD2(float, 8) else BWD2(float, 16)
    }
#undef BWD2
#undef BWD2_A
#undef BWD2_W
    if (want_w)
        launch_embed_finish(part, grid_w, gw1, nullptr, gw2, nullptr, E, stream);
    return check_launch("dg_embed_sym_bwd2_keep");
}
