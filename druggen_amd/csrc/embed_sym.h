// Tile toolbox of the edge-embedding kernels (embed_sym.hip, embed_sym_keep.hip): pair tiles, the layer-1 staging, the
// bf16 x 3 MFMA stages and the layout of the workgroup partial sums.  See embed_sym.hip for the tile program.
#pragma once
#include "bf16.h"
#include "traversal.h"

namespace dg {
// column sums of the backward kernels' workgroup partials into the caller's tensors (embed_sym.hip)
void launch_embed_finish(const float* part, int nblocks, float* dw1, float* db1, float* dw2, float* db2, int E, hipStream_t stream);
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kHid = 64;     // hidden width of the embedding MLP (fixed by the reference)
constexpr int kC = 128;      // output width handled by this kernel
constexpr int kPairs = 32;   // atom pairs per tile
constexpr int kMaxE = 16;
constexpr int kD1Pitch = 68;   // floats per row of the dpre1 tile (16-byte aligned rows, conflict-free b128 reads)

enum Act { kRelu = 0, kLeaky = 1, kSigmoid = 2, kTanh = 3 };

// ACT is a template parameter of the kernels: a run-time switch inside the per-element loops costs a branch ladder
// per value and keeps hipcc from scheduling across the elements
template <int act>
__device__ __forceinline__ float act_fwd(float x) {
    switch (act) {
        case kRelu: return fmaxf(x, 0.f);
        case kLeaky: return x > 0.f ? x : 0.01f * x;
        case kSigmoid: return 1.0f / (1.0f + __expf(-x));
        default: return tanhf(x);
    }
}
// derivative expressed through the OUTPUT y = act(x)
template <int act>
__device__ __forceinline__ float act_grad_from_output(float y) {
    switch (act) {
        case kRelu: return y > 0.f ? 1.f : 0.f;
        case kLeaky: return y > 0.f ? 1.f : 0.01f;
        case kSigmoid: return y * (1.f - y);
        default: return 1.f - y * y;
    }
}
// first and second derivative through the OUTPUT y (embed_sym_smooth.hip); zero curvature for the piecewise-linear ones
template <int act>
__device__ __forceinline__ void act_grad2_from_output(float y, float* d1, float* d2) {
    const float d = act_grad_from_output<act>(y);
    *d1 = d;
    switch (act) {
        case kSigmoid: *d2 = d * fmaf(-2.f, y, 1.f); break;
        case kTanh: *d2 = -2.f * y * d; break;
        default: *d2 = 0.f;
    }
}

struct PairTile {
    int b;        // molecule
    int p0;       // first pair of the tile
};

// pair index p (0 <= p < N(N+1)/2, row-major over i <= j) -> (i, j)
__device__ __forceinline__ void pair_to_ij(int p, int N, int* i_out, int* j_out) {
    int i = 0;
    while (p >= N - i) {
        p -= N - i;
        ++i;
    }
    *i_out = i;
    *j_out = i + p;
}

template <bool BACKWARD>
struct Smem {
    int ij[kPairs][2];
    float a[64][kMaxE];
    float h1[64 * kHid];                          // swizzled [row][64]
};

// Sign words of an edge row (b,i,j), dg_embed_sym_fwd_keep -> dg_embed_sym_bwd_keep / _bwd2_keep: bit (c & 31) of word c >> 5 is
// set iff the layer-2 pre-activation of channel c is > 0 (words 0..3), bit (u & 31) of word 4 + (u >> 5) iff the layer-1
// pre-activation of hidden unit u is (words 4, 5) -- the condition act_grad_from_output(act_fwd(x)) tests.
constexpr int kSignWords = 6;

// Stage the pair table, the input rows and the layer-1 activations of one tile.
// EP = padded number of input features (8 or 16): sizes the per-lane weight / accumulator arrays.
// KEEP: also leave the layer-1 sign words of the 64 tile rows in sg[row][4..5] (a wave holds one row's 64 units per step).
template <int EP, int ACT, bool KEEP = false>
__device__ __forceinline__ void stage_tile(const float* __restrict__ a, const float* __restrict__ w1,
                                           const float* __restrict__ b1, int N, int E, int NP, PairTile t,
                                           int (*ij)[2], float (*at)[kMaxE], float* h1, unsigned* sg = nullptr) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));   // opaque per call: keeps the per-row LDS offsets out of the caller's loop preheader
    if (tid < kPairs) {
        const int p = t.p0 + tid;
        int i = 0, j = 0;
        if (p < NP) pair_to_ij(p, N, &i, &j);
        ij[tid][0] = p < NP ? i : -1;
        ij[tid][1] = j;
    }
    __syncthreads();
    for (int idx = tid; idx < 64 * EP; idx += 256) {
        const int row = idx / EP, e = idx % EP;
        const int pr = row & 31;
        const int i = ij[pr][0], j = ij[pr][1];
        float v = 0.f;
        if (i >= 0 && e < E) {
            const int64_t r = (static_cast<int64_t>(t.b) * N + (row < 32 ? i : j)) * N + (row < 32 ? j : i);
            v = a[r * E + e];
        }
        at[row][e] = v;
    }
    __syncthreads();
    // layer 1: thread = (unit u, row group g of 16 rows)
    const int u = tid & 63, g = tid >> 6;
    float w[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) w[e] = e < E ? w1[u * E + e] : 0.f;
    const float bb = b1[u];
    for (int r = 0; r < 16; ++r) {
        const int row = g * 16 + r;
        float s = bb;
#pragma unroll
        for (int e = 0; e < EP; ++e) s = fmaf(w[e], at[row][e], s);
        h1[row * kHid + (((u >> 2) ^ (row & 15)) << 2) + (u & 3)] = act_fwd<ACT>(s);
        if (KEEP) {
            const unsigned long long m = __builtin_amdgcn_ballot_w64(s > 0.f);
            if (u < 2) sg[row * kSignWords + 4 + u] = static_cast<unsigned>(u ? m >> 32 : m);
        }
    }
    __syncthreads();
}

// ---- bf16 x 3 arithmetic of the MFMA stages (fp32 class) ----------------------------------------------------------
// Every fp32 operand value is split exactly into three bf16 by truncation (h = top 16 bits, m = top 16 bits of x - h,
// l = top 16 bits of x - h - m: together all 24 significand bits) and the six cross products with i + j <= 4 run on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- the arithmetic of the weight-gradient kernel (linear_wgrad.hip).
// 48 MFMAs of 32 cycles per stage instead of 64 fp32 MFMAs of 64 cycles.  LDS tiles stay fp32; fragments are split in
// registers.  Weight operands arrive pre-split ([k-step][plane][lane] x 8 bf16, embed_pack3_kernel).
typedef unsigned u32x4e __attribute__((ext_vector_type(4)));
struct Planes { bf16x8 p[3]; };

__device__ __forceinline__ void split2(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    const unsigned a0 = __float_as_uint(x0), a1 = __float_as_uint(x1);
    h = __builtin_amdgcn_perm(a1, a0, 0x07060302u);
    const float r0 = x0 - __uint_as_float(a0 & 0xFFFF0000u), r1 = x1 - __uint_as_float(a1 & 0xFFFF0000u);
    const unsigned b0 = __float_as_uint(r0), b1 = __float_as_uint(r1);
    m = __builtin_amdgcn_perm(b1, b0, 0x07060302u);
    const float s0 = r0 - __uint_as_float(b0 & 0xFFFF0000u), s1 = r1 - __uint_as_float(b1 & 0xFFFF0000u);
    l = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
}
__device__ __forceinline__ Planes split8(const float (&v)[8]) {
    u32x4e h, m, l;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned hh, mm, ll;
        split2(v[2 * i], v[2 * i + 1], hh, mm, ll);
        h[i] = hh;
        m[i] = mm;
        l[i] = ll;
    }
    Planes r;
    r.p[0] = __builtin_bit_cast(bf16x8, h);
    r.p[1] = __builtin_bit_cast(bf16x8, m);
    r.p[2] = __builtin_bit_cast(bf16x8, l);
    return r;
}
__device__ __forceinline__ Planes split8(const float4& a, const float4& b) {
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    return split8(v);
}
__device__ __forceinline__ f32x16 mfma6(const Planes& a, const Planes& b, f32x16 c) {
    constexpr int TA[6] = {2, 1, 0, 1, 0, 0}, TB[6] = {0, 1, 2, 0, 1, 0};   // smallest terms first
#pragma unroll
    for (int t = 0; t < 6; ++t) c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[TA[t]], b.p[TB[t]], c, 0, 0, 0);
    return c;
}
// The gradient stages (dW2 += dpre2^T h1, dh = dpre2 W2) are backward-only: their roundings travel through linear maps and stay
// roundings, so they take the three leading cross products (m h', h m', h h': 2^-16 of a product left out) -- half
// the MFMAs of a stage.  The layer-2 RECOMPUTATION keeps all six: its signs are the ReLU mask of the forward, which must not flip
// (all three stages on three products: 1.4e-3 .. 4e-3 on the goldens, the square-root law of a perturbed forward).
__device__ __forceinline__ f32x16 mfma_bwd(const Planes& a, const Planes& b, f32x16 c) {
    constexpr int TA[3] = {1, 0, 0}, TB[3] = {0, 1, 0};   // smallest terms first
#pragma unroll
    for (int t = 0; t < 3; ++t) c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[TA[t]], b.p[TB[t]], c, 0, 0, 0);
    return c;
}
// eight consecutive k (chunks c, c + 1 of four floats) of row `row` of an XOR-swizzled fp32 tile with `pitch` floats
__device__ __forceinline__ Planes frag_row(const float* tile, int row, int c, int pitch) {
    const float4 a = ld4(tile + row * pitch + ((c ^ (row & 15)) << 2));
    const float4 b = ld4(tile + row * pitch + (((c + 1) ^ (row & 15)) << 2));
    return split8(a, b);
}
__device__ __forceinline__ Planes load_planes(const bf16x8* p) {   // [plane][lane] of one (tile, k-step)
    Planes r;
#pragma unroll
    for (int q = 0; q < 3; ++q) r.p[q] = p[q * 64];
    return r;
}

// layer 2: this wave's 32-column slab for both orientations, K = 64 = four k-steps.  `w2f` points at the slab's
// pre-split fragments for this lane.
__device__ __forceinline__ void layer2_mfma(const float* h1, const bf16x8* w2f, int lane, f32x16& acc0, f32x16& acc1) {
    const int half = lane >> 5, col = lane & 31;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const Planes b = load_planes(w2f + ks * 3 * 64);
        const Planes a0 = frag_row(h1, col, 4 * ks + 2 * half, kHid);
        const Planes a1 = frag_row(h1, 32 + col, 4 * ks + 2 * half, kHid);
        acc0 = mfma6(a0, b, acc0);
        acc1 = mfma6(a1, b, acc1);
    }
}

// A [32 pairs][128] fp32 LDS tile holds one value per (pair, channel); both orientations (b,i,j) and (b,j,i) of a
// pair receive it as whole rows: one half-wave per row, 16 bytes (fp32) / 8 bytes (bf16) per lane.
template <typename T>
__device__ __forceinline__ void store_pair_rows(const float* xt, const int (*ij)[2], int b, int N, T* __restrict__ out,
                                                int tid) {
    const int hw = tid >> 5, l32 = tid & 31;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int pr = hw + 8 * it;
        const int i = ij[pr][0], j = ij[pr][1];
        if (i < 0) continue;
        const float4 v = ld4(xt + pr * kC + 4 * l32);
        const int64_t base = static_cast<int64_t>(b) * N;
        st4(out + ((base + i) * N + j) * kC + 4 * l32, v);
        if (i != j) st4(out + ((base + j) * N + i) * kC + 4 * l32, v);
    }
}

// global edge row of tile row `row` (rows 0..31: orientation (i,j), rows 32..63: (j,i)) of the pair (i, j)
__device__ __forceinline__ int64_t tile_edge_row(int b, int N, int row, int i, int j) {
    return (static_cast<int64_t>(b) * N + (row < 32 ? i : j)) * N + (row < 32 ? j : i);
}

// W-gradient stage of the backward kernels: aw2[t] += P^T Q over the 64 tile rows (four k-steps of 16 rows), P = the
// wave's 32 output channels of the [64][128] tile `d2`, Q = unit tiles t = 0, 1 of the [64][64] tile `hq`.  Operands are
// gathered column-wise (eight ds_read_b32 per fragment: a lane's eight rows of one column) and split in registers.
__device__ __forceinline__ void aw2_stage(const float* d2, const float* hq, int n, int col, int half, f32x16 (&aw2)[2]) {
    const int c = n >> 2;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        float av[8], b0[8], b1v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = 16 * ks + 8 * half + j;
            av[j] = d2[r * kC + (((c & ~15) | ((c & 15) ^ (r & 15))) << 2) + (n & 3)];
            b0[j] = hq[r * kHid + ((((col) >> 2) ^ (r & 15)) << 2) + (col & 3)];
            b1v[j] = hq[r * kHid + ((((32 + col) >> 2) ^ (r & 15)) << 2) + (col & 3)];
        }
        const Planes pa = split8(av);
        aw2[0] = mfma_bwd(pa, split8(b0), aw2[0]);
        aw2[1] = mfma_bwd(pa, split8(b1v), aw2[1]);
    }
}
// dh1 = P W2 for one (32-row block, 32-unit tile): K = 128 channels = eight k-steps, two accumulator chains
__device__ __forceinline__ f32x16 dh_stage(const float* d2, const bf16x8* w2g, int row, int half) {
    f32x16 d0, d1v;
#pragma unroll
    for (int i = 0; i < 16; ++i) d0[i] = d1v[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 8; ks += 2) {
        d0 = mfma_bwd(frag_row(d2, row, 4 * ks + 2 * half, kC), load_planes(w2g + ks * 3 * 64), d0);
        d1v = mfma_bwd(frag_row(d2, row, 4 * (ks + 1) + 2 * half, kC), load_planes(w2g + (ks + 1) * 3 * 64), d1v);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) d0[i] += d1v[i];
    return d0;
}

// Per-workgroup partial sums of the backward kernels go to `part`, reduced afterwards in a fixed order.
struct BwdPart {
    // floats per workgroup: dW2 [128*64] | db2 [128] | dW1 [64*16] | db1 [64]
    static constexpr int kW2 = 0, kB2 = kC * kHid, kW1 = kB2 + kC, kB1 = kW1 + kHid * kMaxE, kTotal = kB1 + kHid;
};

constexpr int kBwdPerCu = 2;   // backward workgroups per CU (71 KB of LDS each): their serial phases overlap
int embed_grid(int total_tiles, int per_cu) {
    const int cap = 256 * per_cu;
    return total_tiles < cap ? (total_tiles < 1 ? 1 : total_tiles) : cap;
}

bool embed_shape_ok(int N, int E, int H, int C, int act) {
    return N >= 1 && E >= 1 && E <= kMaxE && H == kHid && C == kC && act >= 0 && act <= 3;
}

}  // namespace
}  // namespace dg
