// Batch assembly from a GPU-resident molecule set (druggen_amd/resident.py): what a DataLoader's collate, four
// host -> device copies and dg_densify produce for a batch (reference src/data/utils.py:128-142), from an index tensor.
//   store:  atoms [n, N] u8 (PAD = 0), ptr [n + 1] i64, entries u32 = row | col << 8 | label << 16 -- the non-zeros of a
//           molecule's dense [N, N] bond-label matrix (both directions of a symmetric molecule, (row, col) unique)
//   batch:  labels [B, N, N] i32, a [B, N, N, E] = one-hot(labels), x [B, N, M] = one-hot(atoms[index[b]]) -- EVERY element
//           written, zeros included (the caller allocates with torch.empty)
//
// One workgroup of 256 lanes per output molecule.  Phases: zero the [N, N] label bytes in LDS (<= 64 KiB) -> scatter the
// molecule's entries into them (byte stores, unique targets: no atomics) -> barrier -> stream labels, a and x out of LDS.
// A molecule's base in `a` / `x` / `labels` is only 4-byte aligned in general (N N E = 10 125 at the headline shape), so
// every output stream is cut into a scalar head up to the first 16-byte boundary, 16-byte stores, and a scalar tail.
// The only data-dependent loop bound is the molecule's entry count, clamped to N N; an index outside [0, n) is clamped
// into range and counted in `bad_index` (the one atomic of the kernel, on the error path).
//
// dg_mol_gather_features: the same batch from a store that carries a feature plane next to `atoms` (the reference's
// --features node matrices, dataset.py:305-307): bits [n, N, W] u32, feature f of an atom position = bit f % 32 of word f / 32.
// x [B, N, M] is then one-hot(atoms) in the columns below atom_dim and the bits in the columns from atom_dim up.  The index,
// label and `a` phases are gather_bonds() for both kernels; only the x stream differs.
#include "common.h"

namespace dg {
namespace {

constexpr int MG_THREADS = 256;

typedef int v4i __attribute__((ext_vector_type(4)));

// dst[0..total) = value(k), dst 4-byte aligned: scalar stores up to the first 16-byte boundary, then one 16-byte store per
// lane and round (consecutive lanes, consecutive 16 bytes), then the scalar tail.  value4(k, out) fills four consecutive.
template <typename T, typename V4, typename F1, typename F4>
__device__ __forceinline__ void stream_out(T* __restrict__ dst, int total, int tid, F1 value, F4 value4) {
    int head = static_cast<int>(((16u - (static_cast<unsigned>(reinterpret_cast<uintptr_t>(dst)) & 15u)) & 15u) >> 2);
    head = head < total ? head : total;
    if (tid < head) dst[tid] = value(tid);
    const int nvec = (total - head) >> 2;
    for (int v = tid; v < nvec; v += MG_THREADS) {
        const int k = head + 4 * v;
        V4 out;
        value4(k, out);
        *reinterpret_cast<V4*>(dst + k) = out;
    }
    const int done = head + 4 * nvec;
    if (tid < total - done) dst[done + tid] = value(done + tid);
}

// The phases both kernels share: the clamped molecule of this workgroup, its bond labels through LDS, `labels` and `a` out.
// Returns the molecule (every lane the same value).
__device__ __forceinline__ int64_t gather_bonds(const int64_t* __restrict__ ptr, const uint32_t* __restrict__ entries, int64_t n,
                                                const int64_t* __restrict__ index, int N, int E, float* __restrict__ a,
                                                int* __restrict__ labels, int* __restrict__ bad_index) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lab[];      // [N, N] bond labels, padded to 16 bytes
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int NN = N * N;

    int64_t m = index[b];
    if (m < 0 || m >= n) {
        if (tid == 0) atomicAdd(bad_index, 1);
        m = m < 0 ? 0 : n - 1;
    }

    // ---- zero, scatter, barrier -------------------------------------------------------------------------------------
    uint32_t* lab_words = reinterpret_cast<uint32_t*>(lab);
    for (int w = tid; w < (NN + 3) >> 2; w += MG_THREADS) lab_words[w] = 0u;
    __syncthreads();
    const int64_t first = ptr[m];
    int64_t count = ptr[m + 1] - first;
    count = count < 0 ? 0 : (count > NN ? NN : count);      // a corrupted ptr cannot run away
    for (int k = tid; k < static_cast<int>(count); k += MG_THREADS) {
        const uint32_t w = entries[first + k];
        const int row = w & 255u, col = (w >> 8) & 255u;
        if (row < N && col < N) lab[row * N + col] = static_cast<unsigned char>(w >> 16);      // (never outside the LDS image)
    }
    __syncthreads();

    // ---- labels [N, N] int32 ------------------------------------------------------------------------------------------
    stream_out<int, v4i>(
        labels + b * NN, NN, tid, [&](int k) { return static_cast<int>(lab[k]); },
        [&](int k, v4i& out) {
#pragma unroll
            for (int c = 0; c < 4; ++c) out[c] = lab[k + c];
        });

    // ---- a [N, N, E] one-hot float32: one division per 16-byte store, then (pair, class) advance together ----------------
    stream_out<float, v4f>(
        a + b * NN * E, NN * E, tid, [&](int k) { return lab[k / E] == k % E ? 1.0f : 0.0f; },
        [&](int k, v4f& out) {
            int pair = k / E, cls = k - pair * E;
            int l = lab[pair];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                out[c] = l == cls ? 1.0f : 0.0f;
                if (++cls == E) {
                    cls = 0;
                    ++pair;
                    l = pair < NN ? lab[pair] : 0;
                }
            }
        });
    return m;
}

__global__ __launch_bounds__(MG_THREADS) void mol_gather_kernel(
    const uint8_t* __restrict__ atoms, const int64_t* __restrict__ ptr, const uint32_t* __restrict__ entries, int64_t n,
    const int64_t* __restrict__ index, int N, int M, int E, float* __restrict__ a, int* __restrict__ labels,
    float* __restrict__ x, int* __restrict__ bad_index) {
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t m = gather_bonds(ptr, entries, n, index, N, E, a, labels, bad_index);

    // ---- x [N, M] one-hot float32 of the atom labels (N bytes of the store, read through the caches) ------------------------
    const uint8_t* __restrict__ at = atoms + m * N;
    stream_out<float, v4f>(
        x + b * N * M, N * M, tid, [&](int k) { return at[k / M] == k % M ? 1.0f : 0.0f; },
        [&](int k, v4f& out) {
            int node = k / M, cls = k - node * M;
            int l = at[node];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                out[c] = l == cls ? 1.0f : 0.0f;
                if (++cls == M) {
                    cls = 0;
                    ++node;
                    l = node < N ? at[node] : 0;
                }
            }
        });
}

__global__ __launch_bounds__(MG_THREADS) void mol_gather_features_kernel(
    const uint8_t* __restrict__ atoms, const int64_t* __restrict__ ptr, const uint32_t* __restrict__ entries,
    const uint32_t* __restrict__ bits, int64_t n, const int64_t* __restrict__ index, int N, int M, int E, int W, int A,
    float* __restrict__ a, int* __restrict__ labels, float* __restrict__ x, int* __restrict__ bad_index) {
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t m = gather_bonds(ptr, entries, n, index, N, E, a, labels, bad_index);

    // ---- x [N, M]: columns < A one-hot of the atom label, columns >= A the feature bits (N bytes and N W words of the store,
    // read through the caches).  node < N at every load: k < N M in value(), and value4() steps to a new row only below N.
    const uint8_t* __restrict__ at = atoms + m * N;
    const uint32_t* __restrict__ fb = bits + m * N * W;
    auto element = [&](int l, const uint32_t* __restrict__ row, int col) {
        if (col < A) return l == col ? 1.0f : 0.0f;
        const int f = col - A;
        return (row[f >> 5] >> (f & 31)) & 1u ? 1.0f : 0.0f;
    };
    stream_out<float, v4f>(
        x + b * N * M, N * M, tid,
        [&](int k) {
            const int node = k / M;
            return element(at[node], fb + node * W, k - node * M);
        },
        [&](int k, v4f& out) {
            int node = k / M, col = k - node * M;
            int l = at[node];
            const uint32_t* __restrict__ row = fb + node * W;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                out[c] = element(l, row, col);
                if (++col == M) {
                    col = 0;
                    if (++node < N) {
                        l = at[node];
                        row += W;
                    }
                }
            }
        });
}

}  // namespace
}  // namespace dg

using namespace dg;

extern "C" int dg_mol_gather(const uint8_t* atoms, const int64_t* ptr, const uint32_t* entries, int64_t n,
                             const int64_t* index, int B, int N, int M, int E, float* a, int* labels, float* x,
                             int* bad_index, dg_stream_t stream_) {
    if (B < 0 || N < 1 || N > 256 || M < 1 || M > 255 || E < 1 || E > 16 || n < 0)
        return fail(DG_E_SHAPE, "dg_mol_gather: need B >= 0, 1 <= N <= 256, 1 <= M <= 255, 1 <= E <= 16, n >= 0 (B=%d N=%d M=%d E=%d n=%lld)",
                    B, N, M, E, static_cast<long long>(n));
    if (B == 0) return 0;
    if (!atoms || !ptr || !entries || !index || !a || !labels || !x || !bad_index)
        return fail(DG_E_ARG, "dg_mol_gather: null pointer");
    if (n < 1) return fail(DG_E_SHAPE, "dg_mol_gather: a batch of B=%d molecules needs a store with n >= 1", B);
    if ((reinterpret_cast<uintptr_t>(a) & 3) || (reinterpret_cast<uintptr_t>(labels) & 3) || (reinterpret_cast<uintptr_t>(x) & 3) ||
        (reinterpret_cast<uintptr_t>(entries) & 3) || (reinterpret_cast<uintptr_t>(bad_index) & 3) ||
        (reinterpret_cast<uintptr_t>(ptr) & 7) || (reinterpret_cast<uintptr_t>(index) & 7))
        return fail(DG_E_ARG, "dg_mol_gather: misaligned pointer (a, labels, x, entries, bad_index: 4 bytes; ptr, index: 8)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const hipError_t err = hipMemsetAsync(bad_index, 0, sizeof(int), stream);
    if (err != hipSuccess) return fail(static_cast<int>(err), "dg_mol_gather: %s", hipGetErrorString(err));
    const int lds = (N * N + 15) & ~15;
    DG_OPT_IN_LDS(&mol_gather_kernel, 256 * 256);      // the largest request (N = 256: 64 KiB), set once per device
    hipLaunchKernelGGL(mol_gather_kernel, dim3(static_cast<unsigned>(B)), dim3(MG_THREADS), lds, stream, atoms, ptr, entries, n,
                       index, N, M, E, a, labels, x, bad_index);
    return check_launch("dg_mol_gather");
}

extern "C" int dg_mol_gather_features(const uint8_t* atoms, const int64_t* ptr, const uint32_t* entries, const uint32_t* bits,
                                      int64_t n, const int64_t* index, int B, int N, int M, int E, int W, int atom_dim,
                                      float* a, int* labels, float* x, int* bad_index, dg_stream_t stream_) {
    if (B < 0 || N < 1 || N > 256 || M < 1 || M > 255 || E < 1 || E > 16 || n < 0)
        return fail(DG_E_SHAPE, "dg_mol_gather_features: need B >= 0, 1 <= N <= 256, 1 <= M <= 255, 1 <= E <= 16, n >= 0 (B=%d N=%d M=%d E=%d n=%lld)",
                    B, N, M, E, static_cast<long long>(n));
    if (atom_dim < 1 || atom_dim > M || W != (M - atom_dim + 31) / 32)
        return fail(DG_E_SHAPE, "dg_mol_gather_features: need 1 <= atom_dim <= M and W == ceil((M - atom_dim) / 32) (M=%d atom_dim=%d W=%d)",
                    M, atom_dim, W);
    if (B == 0) return 0;
    if (!atoms || !ptr || !entries || (!bits && W > 0) || !index || !a || !labels || !x || !bad_index)
        return fail(DG_E_ARG, "dg_mol_gather_features: null pointer");
    if (n < 1) return fail(DG_E_SHAPE, "dg_mol_gather_features: a batch of B=%d molecules needs a store with n >= 1", B);
    if ((reinterpret_cast<uintptr_t>(a) & 3) || (reinterpret_cast<uintptr_t>(labels) & 3) || (reinterpret_cast<uintptr_t>(x) & 3) ||
        (reinterpret_cast<uintptr_t>(entries) & 3) || (reinterpret_cast<uintptr_t>(bits) & 3) ||
        (reinterpret_cast<uintptr_t>(bad_index) & 3) || (reinterpret_cast<uintptr_t>(ptr) & 7) ||
        (reinterpret_cast<uintptr_t>(index) & 7))
        return fail(DG_E_ARG, "dg_mol_gather_features: misaligned pointer (a, labels, x, entries, bits, bad_index: 4 bytes; ptr, index: 8)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const hipError_t err = hipMemsetAsync(bad_index, 0, sizeof(int), stream);
    if (err != hipSuccess) return fail(static_cast<int>(err), "dg_mol_gather_features: %s", hipGetErrorString(err));
    const int lds = (N * N + 15) & ~15;
    DG_OPT_IN_LDS(&mol_gather_features_kernel, 256 * 256);
    hipLaunchKernelGGL(mol_gather_features_kernel, dim3(static_cast<unsigned>(B)), dim3(MG_THREADS), lds, stream, atoms, ptr, entries,
                       bits, n, index, N, M, E, W, atom_dim, a, labels, x, bad_index);
    return check_launch("dg_mol_gather_features");
}
