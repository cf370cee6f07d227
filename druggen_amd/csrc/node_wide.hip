// Node-side layers of a --features model (reference dataset.py:305-307: m_dim = atom types + 54 descriptor columns, 67 for the
// ChEMBL encoder; the store's limit is 255):
//   node_layers  Linear(E,64) - act - Linear(64,128) - act   (models.py:52-56, 154-158)   1 <= E <= 255
//   readout_n    Linear(128, N)                              (models.py:100-101)          17 <= N <= 255
// embed_node.hip and the skinny readout keep E, N <= 16 in registers; here the wide dimension is walked in slabs.
//   embed_node_wide_chain   the chain of embed_node.hip with layer 1 over slabs of 32 input columns: bias first, one accumulator
//                           per output, inputs in ascending index, so at E <= 16 it equals dg_embed_node_chain bit for bit.
//                           Layer 2 is embed_node.h's.
//   embed_node_wide_bwd     g2, g1 as in embed_node.hip (embed_node.h); dz = g1 W1 over slabs of 128 columns, W1 staged where
//                           W2 lay.
//   outer_rows              out[a][b] = sum_r A[r][a] B[r][b] (+ column sums of A) over a fixed split of the rows, partial
//                           sums to a workspace, reduced in a fixed order (launch_ln_finish): dW1 = g1^T z with A = g1, B = z;
//                           the readout's dW = dy^T x with A = dy, B = x.
//   wide_linear_fwd / _dgrad   the readout, 32 rows per tile in LDS: one output column per thread against weight slabs in LDS
//                           (forward), one input column per thread against weight rows from the cache (input gradient).
// All arithmetic is float32 fmaf; no atomics: every result is a fixed sequence of operations.
#include "bf16.h"
#include "embed_node.h"

namespace dg {
namespace {

constexpr int kEMax = 255;                      // the resident store's limit on m_dim (mol_gather.hip)
constexpr int kES = 32;                         // layer 1: input columns per slab
constexpr int kS1 = kNodeH + 1;                 // stride of a transposed W1 slab in LDS
constexpr int kZS = 128;                        // dz: columns per slab (a slab of W1 takes W2's place in LDS)

template <int ACT, bool MASKED>
__global__ __launch_bounds__(256) void embed_node_wide_chain_kernel(const float* __restrict__ in, const float* __restrict__ m1,
                                                                    const float* __restrict__ m2, const float* __restrict__ w1,
                                                                    const float* __restrict__ b1, const float* __restrict__ w2,
                                                                    const float* __restrict__ b2, float* __restrict__ o1,
                                                                    float* __restrict__ o2, int64_t R, int E) {
    __shared__ float w1t[kES * kS1];            // [e][j] of the slab
    __shared__ float w2t[kNodeH * kNodeS2];     // [j][i]
    __shared__ float zs[kNodeRows * kES];
    __shared__ __attribute__((aligned(16))) float a1s[kNodeRows * kNodeH];
    const int t = threadIdx.x;
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kNodeRows;
    node_stage_w2t(w2, w2t, t);
    // layer 1: thread (j = t % 64, row group t / 64) -> rows rg, rg + 4, ...; columns past E are zeros (fmaf(0, 0, acc) = acc)
    const int j = t % kNodeH, rg = t / kNodeH;
    float acc[kNodeRows / 4];
    {
        const float bj = (MASKED || !b1) ? 0.f : b1[j];
#pragma unroll
        for (int n = 0; n < kNodeRows / 4; ++n) acc[n] = bj;
    }
    for (int e0 = 0; e0 < E; e0 += kES) {
        if (e0) __syncthreads();      // the slab before is read
        for (int idx = t; idx < kNodeH * kES; idx += 256) {
            const int jj = idx / kES, e = e0 + idx % kES;
            w1t[(idx % kES) * kS1 + jj] = e < E ? w1[jj * E + e] : 0.f;
        }
        for (int idx = t; idx < kNodeRows * kES; idx += 256) {
            const int64_t r = r0 + idx / kES;
            const int e = e0 + idx % kES;
            zs[idx] = (r < R && e < E) ? in[r * E + e] : 0.f;
        }
        __syncthreads();
        float wj[kES];
#pragma unroll
        for (int e = 0; e < kES; ++e) wj[e] = w1t[e * kS1 + j];
#pragma unroll
        for (int n = 0; n < kNodeRows / 4; ++n) {
            const int row = rg + 4 * n;
#pragma unroll
            for (int e = 0; e < kES; ++e) acc[n] = fmaf(zs[row * kES + e], wj[e], acc[n]);
        }
    }
#pragma unroll
    for (int n = 0; n < kNodeRows / 4; ++n) {
        const int row = rg + 4 * n;
        const int64_t r = r0 + row;
        float a = 0.f;
        if (r < R) {
            a = MASKED ? acc[n] * node_dact<ACT>(m1[r * kNodeH + j]) : node_act<ACT>(acc[n]);
            o1[r * kNodeH + j] = a;
        }
        a1s[row * kNodeH + j] = a;
    }
    __syncthreads();
    node_layer2<ACT, MASKED>(a1s, w2t, b2, m2, o2, r0, R, t);
}

template <int ACT>
__global__ __launch_bounds__(256) void embed_node_wide_bwd_kernel(const float* __restrict__ g, const float* __restrict__ a1,
                                                                  const float* __restrict__ a2, const float* __restrict__ w1,
                                                                  const float* __restrict__ w2, float* __restrict__ g2o,
                                                                  float* __restrict__ g1o, float* __restrict__ dzo, int64_t R,
                                                                  int E) {
    __shared__ __attribute__((aligned(16))) float w2s[kNodeC * kNodeH];      // W2 [i][j]; then slabs of W1 [j][kZS]
    __shared__ __attribute__((aligned(16))) float g2s[kNodeRows * kNodeC];
    __shared__ __attribute__((aligned(16))) float g1s[kNodeRows * kNodeH];
    static_assert(kNodeH * kZS <= kNodeC * kNodeH, "a slab of W1 fits where W2 lay");
    const int t = threadIdx.x;
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kNodeRows;
    node_bwd_g2_g1<ACT>(g, a1, a2, w2, g2o, g1o, w2s, g2s, g1s, r0, R, t);
    if (!dzo) return;      // (uniform)
    // dz[row][e] = sum_j g1[row][j] w1[j][e]: thread (column t % 128 of the slab, row half t / 128), 16 rows each
    const int el = t % kZS, rh = t / kZS;
    for (int e0 = 0; e0 < E; e0 += kZS) {
        __syncthreads();      // W2 / the slab before is read; g1s is written
        for (int idx = t; idx < kNodeH * kZS; idx += 256) {
            const int e = e0 + idx % kZS;
            w2s[idx] = e < E ? w1[(idx / kZS) * E + e] : 0.f;
        }
        __syncthreads();
        if (e0 + el >= E) continue;      // (the barriers above are reached by every thread: e0 < E is uniform)
        float acc[kNodeRows / 2];
#pragma unroll
        for (int n = 0; n < kNodeRows / 2; ++n) acc[n] = 0.f;
#pragma unroll 4
        for (int j = 0; j < kNodeH; j += 4) {
            const float wa = w2s[j * kZS + el], wb = w2s[(j + 1) * kZS + el], wc = w2s[(j + 2) * kZS + el],
                        wd = w2s[(j + 3) * kZS + el];
#pragma unroll
            for (int n = 0; n < kNodeRows / 2; ++n) {
                const float4 v = *reinterpret_cast<const float4*>(&g1s[(rh + 2 * n) * kNodeH + j]);
                acc[n] = fmaf(v.x, wa, acc[n]);
                acc[n] = fmaf(v.y, wb, acc[n]);
                acc[n] = fmaf(v.z, wc, acc[n]);
                acc[n] = fmaf(v.w, wd, acc[n]);
            }
        }
#pragma unroll
        for (int n = 0; n < kNodeRows / 2; ++n) {
            const int64_t r = r0 + rh + 2 * n;
            if (r < R) dzo[r * E + e0 + el] = acc[n];
        }
    }
}

// ---- out[a][b] = sum_r A[r][a] B[r][b], bsum[a] = sum_r A[r][a] -----------------------------------------------------------
// grid (row blocks, slabs of 64 b, slabs of 64 a); thread (b = t % 64, a group t / 64) keeps the 16 outputs a = 16 ag + m of
// its column.  A rows are broadcasts from LDS, B rows are read across the lanes; the block's rows are added in ascending
// order into one accumulator per output.  Partial sums: part_w [S][NA][NB], part_b [S][NA].
constexpr int kOT = 64;
constexpr int kOuterBlocks = 128;

int64_t outer_rows_per_block(int64_t R) {
    int64_t rpb = (R + kOuterBlocks - 1) / kOuterBlocks;
    rpb = (rpb + kNodeRows - 1) / kNodeRows * kNodeRows;
    return rpb < kNodeRows ? kNodeRows : rpb;
}
int outer_blocks(int64_t R) { return static_cast<int>((R + outer_rows_per_block(R) - 1) / outer_rows_per_block(R)); }
size_t outer_workspace(int64_t R, int NA, int NB) {
    return R < 1 ? 0 : static_cast<size_t>(outer_blocks(R)) * (static_cast<size_t>(NA) * NB + NA) * sizeof(float);
}

template <typename TB>
__global__ __launch_bounds__(256) void outer_rows_kernel(const float* __restrict__ A, const TB* __restrict__ Bm,
                                                         float* __restrict__ part_w, float* __restrict__ part_b, int64_t R,
                                                         int NA, int NB, int64_t rows_per_block) {
    __shared__ __attribute__((aligned(16))) float as[kNodeRows * kOT];
    __shared__ float bs[kNodeRows * kOT];
    const int t = threadIdx.x;
    const int b = t % kOT, ag = t / kOT;
    const int b0 = blockIdx.y * kOT, a0 = blockIdx.z * kOT;
    const int64_t r_lo = static_cast<int64_t>(blockIdx.x) * rows_per_block;
    int64_t r_hi = r_lo + rows_per_block;
    if (r_hi > R) r_hi = R;
    float acc[kOT / 4];
#pragma unroll
    for (int m = 0; m < kOT / 4; ++m) acc[m] = 0.f;
    float bsum = 0.f;      // threads t < 64 of the first b slab: column a0 + t of A
    for (int64_t r0 = r_lo; r0 < r_hi; r0 += kNodeRows) {
        if (r0 != r_lo) __syncthreads();
        for (int idx = t; idx < kNodeRows * kOT; idx += 256) {
            const int64_t r = r0 + idx / kOT;
            const int c = idx % kOT;
            as[idx] = (r < r_hi && a0 + c < NA) ? A[r * NA + a0 + c] : 0.f;
            bs[idx] = (r < r_hi && b0 + c < NB) ? ld1(Bm + r * NB + b0 + c) : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int row = 0; row < kNodeRows; ++row) {
            const float bv = bs[row * kOT + b];
#pragma unroll
            for (int m = 0; m < kOT / 4; m += 4) {
                const float4 av = *reinterpret_cast<const float4*>(&as[row * kOT + (kOT / 4) * ag + m]);
                acc[m] = fmaf(av.x, bv, acc[m]);
                acc[m + 1] = fmaf(av.y, bv, acc[m + 1]);
                acc[m + 2] = fmaf(av.z, bv, acc[m + 2]);
                acc[m + 3] = fmaf(av.w, bv, acc[m + 3]);
            }
        }
        if (part_b && blockIdx.y == 0 && t < kOT)
            for (int row = 0; row < kNodeRows; ++row) bsum += as[row * kOT + t];
    }
    if (b0 + b < NB) {
        float* pw = part_w + static_cast<size_t>(blockIdx.x) * NA * NB;
#pragma unroll
        for (int m = 0; m < kOT / 4; ++m) {
            const int a = a0 + (kOT / 4) * ag + m;
            if (a < NA) pw[static_cast<size_t>(a) * NB + b0 + b] = acc[m];
        }
    }
    if (part_b && blockIdx.y == 0 && t < kOT && a0 + t < NA) part_b[static_cast<size_t>(blockIdx.x) * NA + a0 + t] = bsum;
}

int outer_rows(const char* who, const float* A, const void* Bm, bool b_bf16, float* dw, float* db, void* workspace,
               size_t workspace_bytes, int64_t R, int NA, int NB, hipStream_t stream) {
    if (workspace_bytes < outer_workspace(R, NA, NB)) return fail(DG_E_WORKSPACE, "%s: workspace too small", who);
    const int S = outer_blocks(R);
    const int64_t rpb = outer_rows_per_block(R);
    float* part_w = static_cast<float*>(workspace);
    float* part_b = db ? part_w + static_cast<size_t>(S) * NA * NB : nullptr;
    const dim3 grid(S, (NB + kOT - 1) / kOT, (NA + kOT - 1) / kOT);
    ProfScope prof(DG_K_LINEAR_WGRAD, stream);
    if (b_bf16)
        hipLaunchKernelGGL(outer_rows_kernel<bf16_t>, grid, dim3(256), 0, stream, A, static_cast<const bf16_t*>(Bm), part_w, part_b,
                           R, NA, NB, rpb);
    else
        hipLaunchKernelGGL(outer_rows_kernel<float>, grid, dim3(256), 0, stream, A, static_cast<const float*>(Bm), part_w, part_b,
                           R, NA, NB, rpb);
    launch_ln_finish(part_w, S, 1, NA * NB, dw, nullptr, stream);
    if (db) launch_ln_finish(part_b, S, 1, NA, db, nullptr, stream);
    return check_launch(who);
}

// ---- the readout, 17 <= N <= 255 ------------------------------------------------------------------------------------------
constexpr int kRK = 128;                        // the readout's input width (dim)

// y[r][n] = b[n] + sum_k x[r][k] w[n][k]: thread = (output column n = t % NT, row group t / NT), NT = 64, 128 or 256 column
// threads for N, its 32 NT / 256 rows of the tile in accumulators.  The weights pass through LDS in slabs of 32 k, transposed
// ([k][n], odd stride); the x tile is read as float4 broadcasts.
constexpr int kRKS = 32;
template <typename T, int NT>
__global__ __launch_bounds__(256) void wide_linear_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ b, float* __restrict__ y, int64_t R,
                                                              int N) {
    constexpr int RG = 256 / NT, NR = kNodeRows / RG, WS = NT + 1;
    __shared__ __attribute__((aligned(16))) float xs[kNodeRows * kRK];
    __shared__ float wt[kRKS * WS];
    const int t = threadIdx.x;
    const int n = t % NT, rg = t / NT;
    const float bn = (n < N && b) ? b[n] : 0.f;
    const int64_t tiles = (R + kNodeRows - 1) / kNodeRows;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * kNodeRows;
        float acc[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) acc[i] = bn;
        for (int k0 = 0; k0 < kRK; k0 += kRKS) {
            __syncthreads();      // the tile / the slab before is read
            if (k0 == 0) {
#pragma unroll
                for (int i = 0; i < kNodeRows * kRK / 1024; ++i) {
                    const int idx = 4 * (t + 256 * i);
                    const int64_t r = r0 + idx / kRK;
                    *reinterpret_cast<float4*>(&xs[idx]) = r < R ? ld4(x + r * kRK + idx % kRK) : f4(0.f);
                }
            }
            for (int idx = t; idx < N * kRKS; idx += 256) wt[(idx % kRKS) * WS + idx / kRKS] = w[(idx / kRKS) * kRK + k0 + idx % kRKS];
            __syncthreads();
            if (n >= N) continue;      // (no barrier is skipped: the loop bounds are uniform)
#pragma unroll 2
            for (int k = 0; k < kRKS; k += 4) {
                const float wa = wt[k * WS + n], wb = wt[(k + 1) * WS + n], wc = wt[(k + 2) * WS + n], wd = wt[(k + 3) * WS + n];
#pragma unroll
                for (int i = 0; i < NR; ++i) {
                    const float4 v = *reinterpret_cast<const float4*>(&xs[(rg + RG * i) * kRK + k0 + k]);
                    acc[i] = fmaf(v.x, wa, acc[i]);
                    acc[i] = fmaf(v.y, wb, acc[i]);
                    acc[i] = fmaf(v.z, wc, acc[i]);
                    acc[i] = fmaf(v.w, wd, acc[i]);
                }
            }
        }
        if (n < N) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int64_t r = r0 + rg + RG * i;
                if (r < R) y[r * N + n] = acc[i];
            }
        }
    }
}

// dx[r][k] = sum_n dy[r][n] w[n][k]: thread (k = t % 128, row half t / 128), 16 rows each; the dy tile in LDS (row stride
// NP = N rounded up to 4, zero filled), w[n][.] read across the lanes (a 512-byte line per n, from the cache after the
// first tile)
template <typename T>
__global__ __launch_bounds__(256) void wide_linear_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                T* __restrict__ dx, int64_t R, int N) {
    __shared__ __attribute__((aligned(16))) float dys[kNodeRows * 256];
    const int t = threadIdx.x;
    const int NP = (N + 3) & ~3;
    const int k = t % kRK, rh = t / kRK;
    const int64_t tiles = (R + kNodeRows - 1) / kNodeRows;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * kNodeRows;
        if (tile != blockIdx.x) __syncthreads();
        for (int idx = t; idx < kNodeRows * NP; idx += 256) {
            const int64_t r = r0 + idx / NP;
            const int n = idx % NP;
            dys[idx] = (r < R && n < N) ? dy[r * N + n] : 0.f;
        }
        __syncthreads();
        float acc[kNodeRows / 2];
#pragma unroll
        for (int i = 0; i < kNodeRows / 2; ++i) acc[i] = 0.f;
        for (int n = 0; n < NP; n += 4) {
            const float wa = w[n * kRK + k], wb = n + 1 < N ? w[(n + 1) * kRK + k] : 0.f,
                        wc = n + 2 < N ? w[(n + 2) * kRK + k] : 0.f, wd = n + 3 < N ? w[(n + 3) * kRK + k] : 0.f;
#pragma unroll
            for (int i = 0; i < kNodeRows / 2; ++i) {
                const float4 v = *reinterpret_cast<const float4*>(&dys[(rh + 2 * i) * NP + n]);
                acc[i] = fmaf(v.x, wa, acc[i]);
                acc[i] = fmaf(v.y, wb, acc[i]);
                acc[i] = fmaf(v.z, wc, acc[i]);
                acc[i] = fmaf(v.w, wd, acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < kNodeRows / 2; ++i) {
            const int64_t r = r0 + rh + 2 * i;
            if (r < R) st1(dx + r * kRK + k, acc[i]);
        }
    }
}

int wide_linear_check(const char* who, int64_t R, int N, int K, int dtype) {
    if (!dtype_ok(dtype)) return fail(DG_E_ARG, "%s: unknown dtype %d", who, dtype);
    if (R < 0 || K != kRK || N < 17 || N > kEMax)
        return fail(DG_E_SHAPE, "%s: unsupported R=%lld N=%d K=%d (17 <= N <= 255, K == 128)", who, static_cast<long long>(R), N, K);
    return 0;
}

int tile_grid(int64_t R) {
    const int64_t tiles = (R + kNodeRows - 1) / kNodeRows;
    return static_cast<int>(tiles < 512 ? tiles : 512);
}

}  // namespace
}  // namespace dg

using namespace dg;

/* see include/druggen_hip.h */
extern "C" int dg_embed_node_wide_chain(const float* in, const float* m1, const float* m2, const float* w1, const float* b1,
                                        const float* w2, const float* b2, float* o1, float* o2, int64_t R, int E, int act,
                                        dg_stream_t stream_) {
    if (!in || !w1 || !w2 || !o1 || !o2) return fail(DG_E_ARG, "dg_embed_node_wide_chain: null pointer");
    if ((m1 != nullptr) != (m2 != nullptr))
        return fail(DG_E_ARG, "dg_embed_node_wide_chain: m1 and m2 are given together (second order) or not at all (forward)");
    if (int st = node_check("dg_embed_node_wide_chain", R, E, kEMax, act, m1 != nullptr)) return st;
    if (R == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(static_cast<unsigned>((R + kNodeRows - 1) / kNodeRows));
#define LAUNCH(A, M) hipLaunchKernelGGL((embed_node_wide_chain_kernel<A, M>), grid, dim3(256), 0, stream, in, m1, m2, w1, b1, w2, b2, o1, o2, R, E)
    if (m1) { if (act == kNodeRelu) LAUNCH(kNodeRelu, true); else LAUNCH(kNodeLeaky, true); }
    else if (act == kNodeRelu) LAUNCH(kNodeRelu, false);
    else if (act == kNodeLeaky) LAUNCH(kNodeLeaky, false);
    else if (act == kNodeSigmoid) LAUNCH(kNodeSigmoid, false);
    else LAUNCH(kNodeTanh, false);
#undef LAUNCH
    return check_launch("dg_embed_node_wide_chain");
}

extern "C" int dg_embed_node_wide_bwd(const float* g, const float* a1, const float* a2, const float* w1, const float* w2,
                                      float* g2, float* g1, float* dz, int64_t R, int E, int act, dg_stream_t stream_) {
    if (!g || !a1 || !a2 || !w1 || !w2 || !g2 || !g1) return fail(DG_E_ARG, "dg_embed_node_wide_bwd: null pointer");
    if (int st = node_check("dg_embed_node_wide_bwd", R, E, kEMax, act)) return st;
    if (R == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(static_cast<unsigned>((R + kNodeRows - 1) / kNodeRows));
#define LAUNCH(A) hipLaunchKernelGGL((embed_node_wide_bwd_kernel<A>), grid, dim3(256), 0, stream, g, a1, a2, w1, w2, g2, g1, dz, R, E)
    if (act == kNodeRelu) LAUNCH(kNodeRelu);
    else if (act == kNodeLeaky) LAUNCH(kNodeLeaky);
    else if (act == kNodeSigmoid) LAUNCH(kNodeSigmoid);
    else LAUNCH(kNodeTanh);
#undef LAUNCH
    return check_launch("dg_embed_node_wide_bwd");
}

extern "C" size_t dg_embed_node_wide_wgrad_workspace_bytes(int64_t R, int E) {
    return (E < 1 || E > kEMax) ? 0 : outer_workspace(R, kNodeH, E);
}

extern "C" int dg_embed_node_wide_wgrad(const float* g1, const float* z, float* dw1, float* db1, void* workspace,
                                        size_t workspace_bytes, int64_t R, int E, dg_stream_t stream_) {
    if (!g1 || !z || !dw1 || !workspace) return fail(DG_E_ARG, "dg_embed_node_wide_wgrad: null pointer");
    if (R < 1 || E < 1 || E > kEMax)
        return fail(DG_E_SHAPE, "dg_embed_node_wide_wgrad: unsupported shape R=%lld E=%d (R >= 1, 1 <= E <= 255)",
                    static_cast<long long>(R), E);
    return outer_rows("dg_embed_node_wide_wgrad", g1, z, false, dw1, db1, workspace, workspace_bytes, R, kNodeH, E,
                      static_cast<hipStream_t>(stream_));
}

extern "C" int dg_wide_linear_fwd(const void* x, const float* w, const float* b, float* y, int64_t R, int N, int K, int dtype,
                                  dg_stream_t stream_) {
    if (!x || !w || !y) return fail(DG_E_ARG, "dg_wide_linear_fwd: null pointer");
    if (int st = wide_linear_check("dg_wide_linear_fwd", R, N, K, dtype)) return st;
    if (R == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
#define LAUNCH(T, NT) hipLaunchKernelGGL((wide_linear_fwd_kernel<T, NT>), dim3(tile_grid(R)), dim3(256), 0, stream, static_cast<const T*>(x), w, b, y, R, N)
    if (dtype == DG_DTYPE_BF16) { if (N <= 64) LAUNCH(bf16_t, 64); else if (N <= 128) LAUNCH(bf16_t, 128); else LAUNCH(bf16_t, 256); }
    else { if (N <= 64) LAUNCH(float, 64); else if (N <= 128) LAUNCH(float, 128); else LAUNCH(float, 256); }
#undef LAUNCH
    return check_launch("dg_wide_linear_fwd");
}

extern "C" int dg_wide_linear_dgrad(const float* dy, const float* w, void* dx, int64_t R, int N, int K, int dtype,
                                    dg_stream_t stream_) {
    if (!dy || !w || !dx) return fail(DG_E_ARG, "dg_wide_linear_dgrad: null pointer");
    if (int st = wide_linear_check("dg_wide_linear_dgrad", R, N, K, dtype)) return st;
    if (R == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (dtype == DG_DTYPE_BF16)
        hipLaunchKernelGGL(wide_linear_dgrad_kernel<bf16_t>, dim3(tile_grid(R)), dim3(256), 0, stream, dy, w, static_cast<bf16_t*>(dx), R, N);
    else
        hipLaunchKernelGGL(wide_linear_dgrad_kernel<float>, dim3(tile_grid(R)), dim3(256), 0, stream, dy, w, static_cast<float*>(dx), R, N);
    return check_launch("dg_wide_linear_dgrad");
}

extern "C" size_t dg_wide_linear_wgrad_workspace_bytes(int64_t R, int N, int K) {
    return (K != kRK || N < 17 || N > kEMax) ? 0 : outer_workspace(R, N, K);
}

extern "C" int dg_wide_linear_wgrad(const float* dy, const void* x, float* dw, float* db, void* workspace, size_t workspace_bytes,
                                    int64_t R, int N, int K, int dtype, dg_stream_t stream_) {
    if (!dy || !x || !dw || !workspace) return fail(DG_E_ARG, "dg_wide_linear_wgrad: null pointer");
    if (int st = wide_linear_check("dg_wide_linear_wgrad", R, N, K, dtype)) return st;
    if (R < 1) return fail(DG_E_SHAPE, "dg_wide_linear_wgrad: R=%lld (R >= 1)", static_cast<long long>(R));
    return outer_rows("dg_wide_linear_wgrad", dy, x, dtype == DG_DTYPE_BF16, dw, db, workspace, workspace_bytes, R, N, K,
                      static_cast<hipStream_t>(stream_));
}
