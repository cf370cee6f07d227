// Row GEMM for any widths (dg_row_gemm_any* of include/druggen_hip.h): y [R,N] = a [R,K] . B (+ bias), float32 rows,
// K and N multiples of 32 in [32, 1024] -- the nn.Linear layers of a model whose --dim / --mlp_ratio are not 128 / 3.
//
// Arithmetic of row_gemm.hip: fp16 hi + lo planes under an exact power-of-two scale per ROW of the activation and per output
// CHANNEL of the weight, three products (w_lo.x_hi, w_hi.x_lo, w_hi.x_hi) on v_mfma_f32_16x16x32_f16 into ONE float32
// accumulator per output element, k-steps in ascending order, inverse scales and bias in the epilogue.  The order of the sums
// depends on K alone: bit-identical results from run to run, and for a row whatever tile it falls in.
//
// A workgroup owns a tile of TR rows, whose planes take K TR 4 bytes of LDS: 64 rows and 4 waves for K <= 256, 32 rows and 8
// waves for wider rows (at most 128 KB of LDS: one workgroup per CU, so it brings the waves that hide latencies itself).
//   phase 1  all threads: the tile's rows HBM -> registers (16-byte buffer loads whose range ends at the last row: rows past
//            R read as zeros), row maximum over the 8 lanes that share a row (DPP), hi / lo planes -> LDS in fragment order
//            [k-octet][row ^ swizzle][16 B].  K <= 256: the row stays in registers between maximum and split; wider rows
//            are shared by two groups of 8 lanes (maxima meet in LDS) and read a second time (from L2).
//   phase 2  work items (32 output channels) x (RB blocks of 16 rows) go round the waves.  Per k-step a wave reads the item's
//            weight fragments (4 x 16 B per lane, from L2: the packed weight of 256 x 768 is 786 KB and fits neither LDS nor
//            registers; three buffers in rotation keep two k-steps in flight) and 2 RB activation fragments from LDS, and
//            issues 6 RB MFMAs.  Swapped product (weights = A operand): a lane ends up with 4 consecutive channels of one
//            row and stores them with one 16-byte buffer store whose range ends at the tile's last row.
#include "common.h"

#include <climits>
#include <type_traits>

#include "f16_scale.h"
#include "lane_reduce.h"

namespace dg {
namespace {

constexpr int kMinDim = 32, kMaxDim = 1024;
constexpr int kHeld = 8;      // 32-float chunks of a row a thread group keeps in registers (K <= 256)

bool dim_ok(int d) { return d >= kMinDim && d <= kMaxDim && d % 32 == 0; }
// fragments (f16x8) of the packed weight: [unit N/32][k-step K/32][channel block 2][plane 2][lane 64], then float inv_cs[N]
__host__ __device__ inline size_t frag_count(int n_out, int k) { return static_cast<size_t>(n_out / 32) * (k / 32) * 256; }

// one workgroup of 64 threads per output channel: channel maximum -> scale, hi / lo octets in fragment order
__global__ __launch_bounds__(64) void row_gemm_any_pack_kernel(const float* __restrict__ w, f16x8* __restrict__ packed, int rows,
                                                               int cols, int mode) {
    const int n_out = mode == 0 ? rows : cols, k = mode == 0 ? cols : rows;
    const int ch = blockIdx.x, lane = threadIdx.x;
    auto at = [&](int kk) { return mode == 0 ? w[static_cast<size_t>(ch) * cols + kk] : w[static_cast<size_t>(kk) * cols + ch]; };
    float m = 0.f;
    for (int kk = lane; kk < k; kk += 64) m = fmaxf(m, fabsf(at(kk)));
    m = xor_max<1>(m);
    const unsigned e = scale_exponent(m);
    const float sc = scale_of(e);
    const int ksteps = k >> 5;
    for (int o = lane; o < (k >> 3); o += 64) {      // octet o: k-step o >> 2, quarter o & 3
        f16x8 hi, lo;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float s = at(8 * o + i) * sc;
            const _Float16 h = static_cast<_Float16>(s);
            hi[i] = h;
            lo[i] = static_cast<_Float16>(s - static_cast<float>(h));
        }
        const size_t base = ((static_cast<size_t>(ch >> 5) * ksteps + (o >> 2)) * 2 + ((ch >> 4) & 1)) * 2;
        const int fl = (o & 3) * 16 + (ch & 15);
        packed[(base + 0) * 64 + fl] = hi;
        packed[(base + 1) * 64 + fl] = lo;
    }
    if (lane == 0) reinterpret_cast<float*>(packed + frag_count(n_out, k))[ch] = inv_scale_of(e);
}

constexpr int threads_of(int TR) { return TR == 64 ? 256 : 512; }

template <int TR, int RB>
__global__ __launch_bounds__(threads_of(TR)) void row_gemm_any_kernel(const float* __restrict__ a, const f16x8* __restrict__ packed,
                                                           const float* __restrict__ bias, float* __restrict__ y, const int64_t R,
                                                           const int K, const int N) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int plane = K * TR * 2;      // bytes of one plane: [K / 8 octets][TR rows][16 B]
    float* const inv_rs = reinterpret_cast<float*>(smem + 2 * plane);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kc = K >> 5;
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * TR;
    const int64_t left = R - r0;
    const int rows = static_cast<int>(left < TR ? left : TR);

    // ------------------------------------------------------------------------------------------------ phase 1
    {
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a) + r0 * K, 0, rows * K * 4, 0x00020000);
        const int gid = tid >> 3, l8 = tid & 7;
        auto amax = [](unsigned m, const float4& v) {
            const float t = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
            const unsigned u = __float_as_uint(t);
            return u > m ? u : m;
        };
        // float4 column 8 c + l8 of row `row`: octet 4 c + (l8 >> 1), half l8 & 1; the row sits at slot row ^ (l8 & 6)
        auto split = [&](int row, int c, const float4& v, float sc) {
            f32x2 xa = f32x2{v.x, v.y} * sc, xb = f32x2{v.z, v.w} * sc;
            const f16x2 ha = __builtin_convertvector(xa, f16x2), hb = __builtin_convertvector(xb, f16x2);
            xa -= __builtin_convertvector(ha, f32x2);
            xb -= __builtin_convertvector(hb, f32x2);
            const f16x2 la = __builtin_convertvector(xa, f16x2), lb = __builtin_convertvector(xb, f16x2);
            char* const p = smem + ((4 * c + (l8 >> 1)) * TR + (row ^ (l8 & 6))) * 16 + (l8 & 1) * 8;
            *reinterpret_cast<u32x2*>(p) = u32x2{__builtin_bit_cast(unsigned, ha), __builtin_bit_cast(unsigned, hb)};
            *reinterpret_cast<u32x2*>(p + plane) = u32x2{__builtin_bit_cast(unsigned, la), __builtin_bit_cast(unsigned, lb)};
        };
        if constexpr (TR == 32) {
            // 64 groups, 32 rows: groups g and g + 32 share row g, one takes the even chunks, one the odd ones; their maxima
            // meet in LDS
            unsigned* const rmax = reinterpret_cast<unsigned*>(inv_rs + TR);
            const int row = gid & 31, par = gid >> 5;
            if (tid < TR) rmax[tid] = 0;
            __syncthreads();
            auto load4 = [&](float4 (&t)[4], int c) {      // chunks c, c + 2, c + 4, c + 6; one past the last repeats chunk `par`
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ci = c + 2 * i < kc ? c + 2 * i : par;
                    t[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                                          rsrc, static_cast<unsigned>((row * K + 32 * ci + 4 * l8) * 4), 0, 0));
                }
            };
            float4 t[4];
            unsigned m = 0;
            for (int c = par; c < kc; c += 8) {
                load4(t, c);
#pragma unroll
                for (int i = 0; i < 4; ++i) m = amax(m, t[i]);
            }
            m = umax_dpp<0xB1>(m);
            m = umax_dpp<0x4E>(m);
            m = umax_dpp<0x141>(m);
            if (l8 == 0) atomicMax(rmax + row, m);
            __syncthreads();
            const unsigned e = scale_exponent(__uint_as_float(rmax[row]));
            if (par == 0 && l8 == 0) inv_rs[row] = inv_scale_of(e);
            const float sc = scale_of(e);
            for (int c = par; c < kc; c += 8) {
                load4(t, c);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (c + 2 * i < kc) split(row, c + 2 * i, t[i], sc);
            }
        } else {
            // 32 groups, 64 rows of at most kHeld chunks (K <= 256): rows g and g + 32 stay in registers between maximum and split
            float4 v[2][kHeld];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int c = 0; c < kHeld; ++c)
                    if (c < kc)
                        v[j][c] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                                                 rsrc, static_cast<unsigned>(((gid + 32 * j) * K + 32 * c + 4 * l8) * 4), 0, 0));
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                unsigned m = 0;
#pragma unroll
                for (int c = 0; c < kHeld; ++c)
                    if (c < kc) m = amax(m, v[j][c]);
                m = umax_dpp<0xB1>(m);
                m = umax_dpp<0x4E>(m);
                m = umax_dpp<0x141>(m);      // the 8 lanes of the row
                const unsigned e = scale_exponent(__uint_as_float(m));
                if (l8 == 0) inv_rs[gid + 32 * j] = inv_scale_of(e);
#pragma unroll
                for (int c = 0; c < kHeld; ++c)
                    if (c < kc) split(gid + 32 * j, c, v[j][c], scale_of(e));
            }
        }
    }
    __syncthreads();

    // ------------------------------------------------------------------------------------------------ phase 2
    const int n = lane & 15, kq = lane >> 4;
    constexpr int G = TR / 16 / RB;      // row groups of a tile
    const int items = (N >> 5) * G;
    const float* __restrict__ const inv_cs = reinterpret_cast<const float*>(packed + static_cast<size_t>(N >> 5) * kc * 256);
    const __amdgpu_buffer_rsrc_t rsrc_y = __builtin_amdgcn_make_buffer_rsrc(y + r0 * N, 0, rows * N * 4, 0x00020000);
    for (int item = w; item < items; item += threads_of(TR) / 64) {
        const int u = item / G, rg = item % G;
        const f16x8* __restrict__ const wp = packed + static_cast<size_t>(u) * kc * 256 + lane;
        // activation fragment of lane (row n of block rb, quarter kq) in k-step ks: octet 4 ks + kq, slot row ^ (2 kq)
        const char* const xp = smem + (kq * TR + ((16 * rg * RB + n) ^ (2 * kq))) * 16;
        // weight fragments [channel block][plane] of three k-steps in rotation: two k-steps are in flight while one is used
        f16x8 wb[3][2][2];
        f32x4 acc[RB][2];
        auto fetch = [&](f16x8 (&b)[2][2], int ks) {
            ks = ks < kc ? ks : kc - 1;
#pragma unroll
            for (int i = 0; i < 4; ++i) b[i >> 1][i & 1] = wp[ks * 256 + i * 64];
        };
        auto step = [&](const f16x8 (&wc)[2][2], const int ks, auto first) {
            f16x8 xh[RB], xl[RB];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const char* const p = xp + ks * (4 * TR * 16) + rb * 256;
                xh[rb] = *reinterpret_cast<const f16x8*>(p);
                xl[rb] = *reinterpret_cast<const f16x8*>(p + plane);
            }
            // smallest terms first; the RB x 2 accumulators in rotation
#pragma unroll
            for (int term = 0; term < 3; ++term)
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) {
                        if (decltype(first)::value && term == 0) mfma16_first(acc[rb][cb], wc[cb][1], xh[rb]);
                        else mfma16(acc[rb][cb], wc[cb][term == 0 ? 1 : 0], term == 1 ? xl[rb] : xh[rb]);
                    }
        };
        fetch(wb[0], 0);
        fetch(wb[1], 1);
        fetch(wb[2], 2);
        step(wb[0], 0, std::true_type{});
        for (int ks = 1; ks < kc; ks += 3) {      // k-step ks reads buffer ks % 3; the buffer of k-step ks - 1 takes k-step ks + 2
            fetch(wb[0], ks + 2);
            step(wb[1], ks, std::false_type{});
            if (ks + 1 < kc) {
                fetch(wb[1], ks + 3);
                step(wb[2], ks + 1, std::false_type{});
            }
            if (ks + 2 < kc) {
                fetch(wb[2], ks + 4);
                step(wb[0], ks + 2, std::false_type{});
            }
        }
        mfma_results_ready();
        // lane (row n of block rb, channel group kq) holds channels 32 u + 16 cb + 4 kq + i of its row
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const int row = 16 * (rg * RB + rb) + n;
            const float rs = inv_rs[row];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const int c0 = 32 * u + 16 * cb + 4 * kq;
                const float4 cs = ld4(inv_cs + c0);
                const float4 bs = bias ? ld4(bias + c0) : f4(0.f);
                const f32x4 v = {fmaf(acc[rb][cb][0], rs * cs.x, bs.x), fmaf(acc[rb][cb][1], rs * cs.y, bs.y),
                                 fmaf(acc[rb][cb][2], rs * cs.z, bs.z), fmaf(acc[rb][cb][3], rs * cs.w, bs.w)};
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrc_y, static_cast<unsigned>((row * N + c0) * 4), 0, 0);
            }
        }
    }
}

constexpr int tile_rows(int K) { return K <= 256 ? 64 : 32; }
constexpr int lds_bytes(int K) { return K * tile_rows(K) * 4 + tile_rows(K) * 8; }      // planes, inverse row scales, row maxima

// Row blocks per work item: the largest of 4 (TR = 64 only), 2, 1 that keeps at least 80 % of the waves' rounds busy, else the
// one that keeps most -- a function of (K, N) alone.
int row_blocks(int K, int N) {
    const int units = N / 32, blocks = tile_rows(K) / 16, nw = threads_of(tile_rows(K)) / 64;
    int best = 1, best_eff = 0;
    for (int rb = blocks; rb >= 1; rb >>= 1) {
        const int items = units * (blocks / rb);
        const int eff = items * 100 / ((items + nw - 1) / nw * nw);
        if (eff >= 80) return rb;
        if (eff > best_eff) {
            best_eff = eff;
            best = rb;
        }
    }
    return best;
}

}  // namespace
}  // namespace dg

using namespace dg;

extern "C" size_t dg_row_gemm_any_packed_bytes(int n_out, int k) {
    if (!dim_ok(n_out) || !dim_ok(k)) return 0;
    return frag_count(n_out, k) * sizeof(f16x8) + static_cast<size_t>(n_out) * sizeof(float);
}

extern "C" int dg_row_gemm_any_pack(const float* w, void* packed, int rows, int cols, int mode, dg_stream_t stream) {
    if (!w || !packed) return fail(DG_E_ARG, "dg_row_gemm_any_pack: null pointer");
    if (mode != 0 && mode != 1) return fail(DG_E_ARG, "dg_row_gemm_any_pack: mode %d (0: forward, 1: input gradient)", mode);
    if (!dim_ok(rows) || !dim_ok(cols))
        return fail(DG_E_SHAPE, "dg_row_gemm_any_pack: unsupported weight [%d,%d] (multiples of 32 in [32, 1024])", rows, cols);
    hipLaunchKernelGGL(row_gemm_any_pack_kernel, dim3(mode == 0 ? rows : cols), dim3(64), 0, static_cast<hipStream_t>(stream), w,
                       static_cast<f16x8*>(packed), rows, cols, mode);
    return check_launch("dg_row_gemm_any_pack");
}

extern "C" int dg_row_gemm_any(const float* a, const void* packed, const float* bias, float* y, int64_t R, int K, int N,
                               dg_stream_t stream) {
    if (!a || !packed || !y) return fail(DG_E_ARG, "dg_row_gemm_any: null pointer");
    if (R < 0 || !dim_ok(K) || !dim_ok(N))
        return fail(DG_E_SHAPE, "dg_row_gemm_any: unsupported shape R=%lld K=%d N=%d (R >= 0; K, N multiples of 32 in [32, 1024])",
                    static_cast<long long>(R), K, N);
    if (R == 0) return 0;
    const int TR = tile_rows(K);
    const int64_t tiles = (R + TR - 1) / TR;
    if (tiles > INT_MAX) return fail(DG_E_SHAPE, "dg_row_gemm_any: R=%lld is more rows than one launch covers", static_cast<long long>(R));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const f16x8* pk = static_cast<const f16x8*>(packed);
    const int rb = row_blocks(K, N);
#define DG_ANY_LAUNCH(TR_, RB_)                                                                                          \
    {                                                                                                                    \
        DG_OPT_IN_LDS((&row_gemm_any_kernel<TR_, RB_>), lds_bytes(TR_ == 64 ? 256 : kMaxDim));                           \
        hipLaunchKernelGGL((row_gemm_any_kernel<TR_, RB_>), dim3(static_cast<unsigned>(tiles)), dim3(threads_of(TR_)), lds_bytes(K), s, a, pk, \
                           bias, y, R, K, N);                                                                            \
    }
    if (TR == 64) {
        if (rb == 4) DG_ANY_LAUNCH(64, 4)
        else if (rb == 2) DG_ANY_LAUNCH(64, 2)
        else DG_ANY_LAUNCH(64, 1)
    } else {
        if (rb == 2) DG_ANY_LAUNCH(32, 2)
        else DG_ANY_LAUNCH(32, 1)
    }
#undef DG_ANY_LAUNCH
    return check_launch("dg_row_gemm_any");
}
