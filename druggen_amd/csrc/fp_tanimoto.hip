// Tanimoto similarity of packed bit fingerprints, aggregated over a stock set for every generated row (reference
// src/util/utils.py:550-611, `average_agg_tanimoto` / `internal_diversity`: dense float32 torch.mm in 5000 x 5000 blocks on
// the host).  Packed layout: [n, W] 32-bit words, W = nbits / 32, bit k of a fingerprint = bit k % 32 of word k / 32.
//   c = popcount(stock[s] & gen[g]),  q(s, g) = float32(c) / float32(a_s + b_g - c)  (1 when the denominator is 0)
//   max mode : out[g] = max_s q (float32), idx[g] = the smallest s that attains it
//   mean mode: out[g] = (sum_s q, accumulated in float64) / S
// Every result is a fixed-order function of the inputs: no atomics, the same bits on every run and stream.
//
// One wave per 64 gen rows x one slice of the stock.  A lane keeps ITS gen row in registers (W VGPRs); the stock row is the
// same for all 64 lanes, so it is read with wave-uniform loads into SGPRs and enters `v_and_b32` as its scalar operand:
// a pair costs W x (v_and_b32 + v_bcnt_u32_b32, which adds into the running count) and no LDS traffic, no barrier.
// In max mode the IEEE division runs only when some lane may have a new maximum: c / d > cb / db is decided exactly by
// c db > cb d in 24-bit integer products, and rounding is monotone, so a fraction that is not larger cannot give a
// larger float32 quotient.  Mean mode divides every pair (each term is the float32 quotient by definition).
//
// The stock is cut into `nsplit` slices (grid y) so that a handful of gen rows against a million stock rows still fills
// the chip; slice results go to the workspace and a second launch folds them in ascending slice order.
#include "common.h"

namespace dg {
namespace {

constexpr int FPT_WAVE = 64;
constexpr int FPT_TARGET_WAVES = 16384;      // 256 CUs x 4 SIMDs x 16: several rounds of waves, so the last round is a small tail
constexpr int FPT_MIN_ROWS = 128;            // slices are capped at ceil(S / 128): about 128 stock rows or more each (never under 64)
constexpr int FPT_MAX_SPLITS = 65535;        // grid y

struct Split {
    int n;         // slices
    int rows;      // stock rows per slice (the last one may be shorter, never empty)
};

// Depends on the shapes alone (not on the device), so the summation order of mean mode is a property of (S, G).
Split split_of(int64_t S, int64_t G) {
    const int64_t gblocks = (G + FPT_WAVE - 1) / FPT_WAVE;
    int64_t n = (FPT_TARGET_WAVES + gblocks - 1) / gblocks;
    const int64_t cap = (S + FPT_MIN_ROWS - 1) / FPT_MIN_ROWS;
    if (n > cap) n = cap;
    if (n > FPT_MAX_SPLITS) n = FPT_MAX_SPLITS;
    if (n < 1) n = 1;
    const int64_t rows = (S + n - 1) / n;
    return Split{static_cast<int>((S + rows - 1) / rows), static_cast<int>(rows)};
}

// d == 0 only with c == 0 (both rows empty): 0 / 0 becomes 1 / 1 without a branch.  The division is the correctly rounded
// one: this build has no fast-math.
__device__ __forceinline__ float quotient(int c, int d) {
    const int z = d == 0;
    return static_cast<float>(c + z) / static_cast<float>(d + z);
}

// WP: gen words held per lane (W <= WP; EXACT: W == WP, no per-word bound test).
template <int WP, bool EXACT, bool MEAN>
__global__ __launch_bounds__(FPT_WAVE) void fp_tanimoto_kernel(
    const unsigned* __restrict__ stock, const int* __restrict__ stock_counts, const unsigned* __restrict__ gen,
    const int* __restrict__ gen_counts, int S, int G, int W, int rows, int nsplit, float* __restrict__ out_max,
    int* __restrict__ out_idx, double* __restrict__ out_mean, float* __restrict__ part_max, int* __restrict__ part_idx,
    double* __restrict__ part_sum) {
    const int g = blockIdx.x * FPT_WAVE + threadIdx.x;
    const bool live = g < G;
    const int split = blockIdx.y;
    const int s0 = split * rows, s1 = min(S, s0 + rows);

    unsigned gw[WP];
    const unsigned* grow = gen + static_cast<size_t>(live ? g : 0) * W;
#pragma unroll
    for (int k = 0; k < WP; ++k) gw[k] = (EXACT || k < W) ? grow[k] : 0u;      // a lane past G holds row 0 and stores nothing
    const int b = gen_counts[live ? g : 0];

    float best = -1.0f;
    int arg = 0, cb = -1, db = 1;      // cb / db: the fraction behind `best`; -1 / 1 loses to every pair
    double sum = 0.0;

    for (int s = s0; s < s1; ++s) {
        const unsigned* __restrict__ row = stock + static_cast<size_t>(s) * W;      // wave-uniform: SGPR loads
        const int a = stock_counts[s];
        int c = 0;
#pragma unroll
        for (int k = 0; k < WP; ++k) {
            if (EXACT || k < W) c += __popc(row[k] & gw[k]);
        }
        const int d = a + b - c;
        if (MEAN) {
            sum += static_cast<double>(quotient(c, d));
        } else {
            // a == 0 (an empty stock row, wave-uniform): d may be 0 and the quotient 1, which the products cannot see
            const bool maybe = __mul24(c, db) > __mul24(cb, d);
            if (a == 0 || __builtin_amdgcn_ballot_w64(maybe) != 0ull) {
                const float q = quotient(c, d);
                if (q > best) {
                    best = q;
                    arg = s;
                    cb = d ? c : 1;
                    db = d ? d : 1;
                }
            }
        }
    }
    if (!live) return;
    if (nsplit == 1) {
        if (MEAN) {
            out_mean[g] = sum / static_cast<double>(S);
        } else {
            out_max[g] = best;
            if (out_idx) out_idx[g] = arg;
        }
    } else {
        const size_t at = static_cast<size_t>(split) * G + g;
        if (MEAN) {
            part_sum[at] = sum;
        } else {
            part_max[at] = best;
            part_idx[at] = arg;
        }
    }
}

// Slices in ascending order: the first slice that holds the maximum wins (its own index is already its smallest).
template <bool MEAN>
__global__ __launch_bounds__(256) void fp_tanimoto_combine_kernel(const float* __restrict__ part_max,
                                                                  const int* __restrict__ part_idx,
                                                                  const double* __restrict__ part_sum, int S, int G,
                                                                  int nsplit, float* __restrict__ out_max,
                                                                  int* __restrict__ out_idx, double* __restrict__ out_mean) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    if (MEAN) {
        double sum = 0.0;
        for (int p = 0; p < nsplit; ++p) sum += part_sum[static_cast<size_t>(p) * G + g];
        out_mean[g] = sum / static_cast<double>(S);
    } else {
        float best = -1.0f;
        int arg = 0;
        for (int p = 0; p < nsplit; ++p) {
            const float q = part_max[static_cast<size_t>(p) * G + g];
            if (q > best) {
                best = q;
                arg = part_idx[static_cast<size_t>(p) * G + g];
            }
        }
        out_max[g] = best;
        if (out_idx) out_idx[g] = arg;
    }
}

// Dense 0/1 rows -> packed words and bit counts.  One wave per row: 64 consecutive elements per step (coalesced), the
// ballot of "element != 0" IS two packed words.  The count is a wave-uniform sum of popcounts; lane 0 stores.  float32 is
// tested on its bits (everything but +-0 is a set bit: denormals, infinities and NaN too, whatever the denormal mode).
template <typename T, unsigned MASK>
__global__ __launch_bounds__(256) void fp_pack_kernel(const T* __restrict__ dense, int64_t n, int nbits,
                                                      unsigned* __restrict__ words, int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const T* row = dense + r * nbits;
    unsigned* wrow = words + r * (nbits >> 5);
    int count = 0;
    for (int k0 = 0; k0 < nbits; k0 += 64) {
        const int k = k0 + lane;
        const bool bit = k < nbits && (row[k] & MASK) != 0u;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(bit);
        count += __popcll(m);
        if (lane == 0) {
            wrow[k0 >> 5] = static_cast<unsigned>(m);
            if (k0 + 32 < nbits) wrow[(k0 >> 5) + 1] = static_cast<unsigned>(m >> 32);
        }
    }
    if (lane == 0) counts[r] = count;
}

template <int WP, bool EXACT>
void launch_main(bool mean, dim3 grid, hipStream_t st, const unsigned* stock, const int* sc, const unsigned* gen, const int* gc,
                 int S, int G, int W, int rows, int nsplit, float* om, int* oi, double* od, float* pm, int* pi, double* ps) {
    if (mean)
        hipLaunchKernelGGL((fp_tanimoto_kernel<WP, EXACT, true>), grid, dim3(FPT_WAVE), 0, st, stock, sc, gen, gc, S, G, W, rows,
                           nsplit, om, oi, od, pm, pi, ps);
    else
        hipLaunchKernelGGL((fp_tanimoto_kernel<WP, EXACT, false>), grid, dim3(FPT_WAVE), 0, st, stock, sc, gen, gc, S, G, W, rows,
                           nsplit, om, oi, od, pm, pi, ps);
}

bool nbits_ok(int nbits) { return nbits >= 32 && nbits <= 4096 && nbits % 32 == 0; }

}  // namespace
}  // namespace dg

using namespace dg;

extern "C" size_t dg_fp_tanimoto_workspace_bytes(int64_t S, int64_t G) {
    if (S <= 0 || G <= 0 || S > INT32_MAX || G > INT32_MAX) return 0;
    const Split sp = split_of(S, G);
    return sp.n > 1 ? static_cast<size_t>(sp.n) * static_cast<size_t>(G) * 8 : 0;
}

extern "C" int dg_fp_pack(const void* dense, int dtype, int64_t n, int nbits, unsigned* words, int* counts,
                          dg_stream_t stream_) {
    if (!nbits_ok(nbits) || n < 0 || (n + 3) / 4 > INT32_MAX)
        return fail(DG_E_SHAPE, "dg_fp_pack: need n >= 0 and nbits a multiple of 32 in 32..4096 (n=%lld nbits=%d)",
                    static_cast<long long>(n), nbits);
    if (dtype != DG_FP_DENSE_U8 && dtype != DG_FP_DENSE_F32) return fail(DG_E_ARG, "dg_fp_pack: dtype %d is neither DG_FP_DENSE_U8 nor DG_FP_DENSE_F32", dtype);
    if (n == 0) return 0;
    if (!dense || !words || !counts) return fail(DG_E_ARG, "dg_fp_pack: null pointer");
    if ((reinterpret_cast<uintptr_t>(words) & 3) || (reinterpret_cast<uintptr_t>(counts) & 3) ||
        (dtype == DG_FP_DENSE_F32 && (reinterpret_cast<uintptr_t>(dense) & 3)))
        return fail(DG_E_ARG, "dg_fp_pack: words, counts and float32 input must be 4-byte aligned");
    const dim3 grid(static_cast<unsigned>((n + 3) / 4));
    hipStream_t st = static_cast<hipStream_t>(stream_);
    if (dtype == DG_FP_DENSE_U8)
        hipLaunchKernelGGL((fp_pack_kernel<unsigned char, 0xFFu>), grid, dim3(256), 0, st, static_cast<const unsigned char*>(dense), n,
                           nbits, words, counts);
    else
        hipLaunchKernelGGL((fp_pack_kernel<unsigned, 0x7FFFFFFFu>), grid, dim3(256), 0, st, static_cast<const unsigned*>(dense), n,
                           nbits, words, counts);
    return check_launch("dg_fp_pack");
}

extern "C" int dg_fp_tanimoto(const unsigned* stock, const int* stock_counts, int64_t S, const unsigned* gen,
                              const int* gen_counts, int64_t G, int nbits, int mode, void* out, int* idx, void* workspace,
                              size_t workspace_bytes, dg_stream_t stream_) {
    if (!nbits_ok(nbits) || S < 0 || G < 0 || S > INT32_MAX || G > INT32_MAX)
        return fail(DG_E_SHAPE, "dg_fp_tanimoto: need 0 <= S, G < 2^31 and nbits a multiple of 32 in 32..4096 (S=%lld G=%lld nbits=%d)",
                    static_cast<long long>(S), static_cast<long long>(G), nbits);
    if (mode != DG_FP_MAX && mode != DG_FP_MEAN) return fail(DG_E_ARG, "dg_fp_tanimoto: mode %d is neither DG_FP_MAX nor DG_FP_MEAN", mode);
    if (mode == DG_FP_MEAN && idx) return fail(DG_E_ARG, "dg_fp_tanimoto: idx belongs to DG_FP_MAX");
    if (S == 0 || G == 0) return 0;
    if (!stock || !stock_counts || !gen || !gen_counts || !out) return fail(DG_E_ARG, "dg_fp_tanimoto: null pointer");
    const bool mean = mode == DG_FP_MEAN;
    if ((reinterpret_cast<uintptr_t>(stock) & 3) || (reinterpret_cast<uintptr_t>(gen) & 3) ||
        (reinterpret_cast<uintptr_t>(stock_counts) & 3) || (reinterpret_cast<uintptr_t>(gen_counts) & 3) ||
        (reinterpret_cast<uintptr_t>(idx) & 3) || (reinterpret_cast<uintptr_t>(out) & (mean ? 7 : 3)))
        return fail(DG_E_ARG, "dg_fp_tanimoto: words, counts and idx must be 4-byte aligned, out as its element type");
    const Split sp = split_of(S, G);
    const size_t cells = static_cast<size_t>(sp.n) * static_cast<size_t>(G);
    float* pm = nullptr;
    int* pi = nullptr;
    double* ps = nullptr;
    if (sp.n > 1) {
        if (!workspace) return fail(DG_E_ARG, "dg_fp_tanimoto: null pointer (workspace)");
        if (reinterpret_cast<uintptr_t>(workspace) & 7) return fail(DG_E_ARG, "dg_fp_tanimoto: workspace must be 8-byte aligned");
        if (workspace_bytes < cells * 8)
            return fail(DG_E_WORKSPACE, "dg_fp_tanimoto: workspace %zu < %zu bytes", workspace_bytes, cells * 8);
        ps = static_cast<double*>(workspace);
        pm = static_cast<float*>(workspace);
        pi = static_cast<int*>(workspace) + cells;
    }
    float* om = mean ? nullptr : static_cast<float*>(out);
    double* od = mean ? static_cast<double*>(out) : nullptr;
    const int Si = static_cast<int>(S), Gi = static_cast<int>(G), W = nbits / 32;
    const dim3 grid(static_cast<unsigned>((G + FPT_WAVE - 1) / FPT_WAVE), static_cast<unsigned>(sp.n));
    hipStream_t st = static_cast<hipStream_t>(stream_);
#define DG_FPT_GO(WP, EXACT) launch_main<WP, EXACT>(mean, grid, st, stock, stock_counts, gen, gen_counts, Si, Gi, W, sp.rows, sp.n, om, idx, od, pm, pi, ps)
    if (W == 32) DG_FPT_GO(32, true);
    else if (W == 64) DG_FPT_GO(64, true);
    else if (W <= 8) DG_FPT_GO(8, false);
    else if (W < 32) DG_FPT_GO(32, false);
    else if (W < 64) DG_FPT_GO(64, false);
    else DG_FPT_GO(128, false);
#undef DG_FPT_GO
    if (int e = check_launch("dg_fp_tanimoto")) return e;
    if (sp.n > 1) {
        const dim3 cgrid(static_cast<unsigned>((G + 255) / 256));
        if (mean)
            hipLaunchKernelGGL(fp_tanimoto_combine_kernel<true>, cgrid, dim3(256), 0, st, pm, pi, ps, Si, Gi, sp.n, om, idx, od);
        else
            hipLaunchKernelGGL(fp_tanimoto_combine_kernel<false>, cgrid, dim3(256), 0, st, pm, pi, ps, Si, Gi, sp.n, om, idx, od);
        return check_launch("dg_fp_tanimoto (combine)");
    }
    return 0;
}
