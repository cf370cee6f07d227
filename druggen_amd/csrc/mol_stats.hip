// Per-molecule statistics of a decoded batch (dg_mol_stats of include/druggen_hip.h): what the reference's
// logging() (src/util/utils.py:241-355) reads off the generated molecules that is integer arithmetic on the decoded labels
// -- distinct atom types (Metrics.mean_atom_type, utils.py:112-127), over-valent atoms, positions that differ from the
// step's input graph, and the first earlier molecule of the batch with the same decoded graph.  Integers only: every
// output is exact and independent of wave timing; the only atomics are integer adds / ors / mins.
//
// Three launches on the caller's stream:
//   mol_stats_rows   one workgroup of 256 lanes per molecule: columns 0..6 of mol[b, :] and the molecule's 64-bit key
//   mol_stats_dups   one workgroup per molecule b: scan_equal of mol_key.h over the keys of all j < b, every key match
//                    verified by comparing the bytes; column 7 = the smallest verified j
//   mol_stats_totals one workgroup: tot[16] from mol[B, 8]
// Every element of mol and tot is stored by every call; the key workspace is rewritten before it is read.
#include "common.h"
#include "mol_key.h"

namespace dg {
namespace {

constexpr int MST_THREADS = MOL_THREADS;
constexpr int MST_COLS = 8;
constexpr int MST_TOT = 16;

// Key positions (mix of mol_key.h): atom i -> i, n_bonds -> 256, bond row k -> 257 + k.

__global__ __launch_bounds__(MST_THREADS) void mol_stats_rows(
    const unsigned char* __restrict__ atoms, const unsigned* __restrict__ bonds, const int* __restrict__ n_bonds,
    const int* __restrict__ n_components, const int* __restrict__ largest_size, const unsigned short* __restrict__ valence2,
    const unsigned char* __restrict__ in_atoms, const int* __restrict__ in_labels,
    const unsigned short* __restrict__ max_valence2, int N, int cap, int M, unsigned long long key_mask,
    int* __restrict__ mol, unsigned long long* __restrict__ keys) {
    __shared__ unsigned seen[8];                  // bit a: the atom label a occurs
    __shared__ int sums[3];                       // over_valent, changed_atoms, changed_bonds
    __shared__ unsigned long long key;

    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t b = blockIdx.x;
    if (tid < 8) seen[tid] = 0u;
    if (tid < 3) sums[tid] = 0;
    if (tid == 0) key = 0ull;
    __syncthreads();

    const int nb = n_bonds[b];
    const bool truncated = nb > cap;
    const int kept = max(0, min(nb, cap));
    const bool with_valence = valence2 && max_valence2;
    int over = 0, d_atoms = 0, d_bonds = 0;
    unsigned long long h = 0ull;

    if (tid < N) {
        const unsigned a = atoms[b * N + tid];
        atomicOr(&seen[a >> 5], 1u << (a & 31));
        h += mix(tid, a);
        // a label past the table has no limit (0xFFFF never is exceeded by a uint16 either)
        if (with_valence && a < static_cast<unsigned>(M)) over = valence2[b * N + tid] > max_valence2[a];
        if (in_atoms) d_atoms = in_atoms[b * N + tid] != a;
    }
    if (tid == 0) h += mix(256u, static_cast<unsigned>(nb));

    // the bond list: hashed row by row; against the input labels a listed pair (i, j, l) differs when in[i, j] != l
    const unsigned* list = bonds + b * cap;
    const int* in = in_labels ? in_labels + b * N * N : nullptr;
    for (int k = tid; k < kept; k += MST_THREADS) {
        const unsigned row = list[k];
        h += mix(257u + k, row);
        if (in && !truncated) {
            const int i = row & 255u, j = (row >> 8) & 255u, l = (row >> 16) & 255u;
            const int was = (i < N && j < N) ? in[i * N + j] : 0;      // (the decode never lists an atom >= N)
            // ... and every input bond i > j is counted below, so a listed one is taken out here
            d_bonds += (was != l) - (was != 0);
        }
    }
    if (in && !truncated) {
        for (int p = tid; p < N * N; p += MST_THREADS) {
            const int i = p / N, j = p - i * N;
            if (j < i && in[p] != 0) ++d_bonds;
        }
    }

    over = wave_sum(over);
    d_atoms = wave_sum(d_atoms);
    d_bonds = wave_sum(d_bonds);
    h = wave_sum(h);
    if (lane == 0) {
        atomicAdd(&sums[0], over);
        atomicAdd(&sums[1], d_atoms);
        atomicAdd(&sums[2], d_bonds);
        atomicAdd(&key, h);
    }
    __syncthreads();
    if (tid == 0) {
        int types = 0;
        for (int w = 0; w < 8; ++w) types += __popc(seen[w]);
        int* row = mol + b * MST_COLS;
        row[0] = types;
        row[1] = largest_size[b];
        row[2] = n_components[b];
        row[3] = nb;
        row[4] = with_valence ? sums[0] : -1;
        row[5] = in_atoms ? sums[1] : -1;
        row[6] = (in && !truncated) ? sums[2] : -1;
        keys[b] = key & key_mask;
    }
}

__global__ __launch_bounds__(MST_THREADS) void mol_stats_dups(
    const unsigned char* __restrict__ atoms, const unsigned* __restrict__ bonds, const int* __restrict__ n_bonds, int N,
    int cap, const unsigned long long* __restrict__ keys, int* __restrict__ mol) {
    __shared__ int first;
    const int b = blockIdx.x;
    const int nb = n_bonds[b];
    if (nb > cap) {                               // truncated: its list is incomplete (uniform over the workgroup)
        if (threadIdx.x == 0) mol[static_cast<int64_t>(b) * MST_COLS + 7] = -2;
        return;
    }
    // the positional data as one side of a comparison: N atoms for everyone, nobody refused (n_bonds[j] == nb <= cap: a
    // candidate j is not truncated either); the keys are masked already
    const Forms all{nullptr, n_bonds, nullptr, atoms, bonds, cap};
    const int dup = scan_equal(all, reinterpret_cast<const long long*>(keys), nullptr, 0, b, ~0ull, keys[b], N, nb,
                               atoms + static_cast<int64_t>(b) * N, bonds + static_cast<int64_t>(b) * cap, cap, N, &first);
    if (threadIdx.x == 0) mol[static_cast<int64_t>(b) * MST_COLS + 7] = dup < b ? dup : -1;
}

__global__ __launch_bounds__(MST_THREADS) void mol_stats_totals(const int* __restrict__ mol, const int* __restrict__ n_bonds,
                                                                int B, int cap, long long* __restrict__ tot) {
    unsigned long long part[12] = {};             // tot[1 .. 12]
    for (int64_t b = threadIdx.x; b < B; b += MST_THREADS) {
        const int4 lo = *reinterpret_cast<const int4*>(mol + b * MST_COLS);
        const int4 hi = *reinterpret_cast<const int4*>(mol + b * MST_COLS + 4);
        const int col[MST_COLS] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int c = 0; c < 7; ++c)
            if (col[c] >= 0) part[c] += static_cast<unsigned>(col[c]);
        part[7] += col[4] > 0;                    // molecules with an over-valent atom
        part[8] += col[5] == 0 && col[6] == 0;    // copies of their input
        part[9] += col[7] == -1;                  // first of their kind
        part[10] += n_bonds[b] > cap;             // truncated
        part[11] += col[2] == 1;                  // connected
    }
    store_totals<MST_TOT>(part, B, tot);
}

}  // namespace
}  // namespace dg

using namespace dg;

extern "C" size_t dg_mol_stats_workspace_bytes(int B) { return B > 0 ? static_cast<size_t>(B) * 8 : 0; }

extern "C" int dg_mol_stats(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds, const int* n_components,
                            const int* largest_size, const unsigned short* valence2, const unsigned char* in_atoms,
                            const int* in_labels, const unsigned short* max_valence2, int B, int N, int cap, int M,
                            int key_bits, int* mol, int64_t* tot, void* workspace, size_t workspace_bytes,
                            dg_stream_t stream_) {
    if (B < 0 || N < 1 || N > 256 || cap < 0)
        return fail(DG_E_SHAPE, "dg_mol_stats: need B >= 0, 1 <= N <= 256, cap >= 0 (B=%d N=%d cap=%d)", B, N, cap);
    if (max_valence2 && (M < 1 || M > 256))
        return fail(DG_E_SHAPE, "dg_mol_stats: max_valence2 holds 1..256 entries (M=%d)", M);
    if (key_bits < 1 || key_bits > 64) return fail(DG_E_ARG, "dg_mol_stats: key_bits must be in 1..64 (got %d)", key_bits);
    if (!tot || (B > 0 && (!atoms || !n_bonds || !n_components || !largest_size || !mol || !workspace)))
        return fail(DG_E_ARG, "dg_mol_stats: null pointer");
    if (B > 0 && cap > 0 && !bonds) return fail(DG_E_ARG, "dg_mol_stats: null pointer (bonds with cap > 0)");
    if (misaligned(bonds, 4) || misaligned(mol, 16) || misaligned(tot, 8) || misaligned(workspace, 8))
        return fail(DG_E_ARG, "dg_mol_stats: bonds must be 4-byte, mol 16-byte, tot and workspace 8-byte aligned");
    if (workspace_bytes < dg_mol_stats_workspace_bytes(B))
        return fail(DG_E_WORKSPACE, "dg_mol_stats: workspace of %zu bytes, need %zu", workspace_bytes,
                    dg_mol_stats_workspace_bytes(B));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const unsigned long long mask = key_bits == 64 ? ~0ull : (1ull << key_bits) - 1ull;
    auto* keys = static_cast<unsigned long long*>(workspace);
    const unsigned* rows = reinterpret_cast<const unsigned*>(bonds);
    if (B > 0) {
        hipLaunchKernelGGL(mol_stats_rows, dim3(static_cast<unsigned>(B)), dim3(MST_THREADS), 0, stream, atoms, rows, n_bonds,
                           n_components, largest_size, valence2, in_atoms, in_labels, max_valence2, N, cap, M, mask, mol, keys);
        hipLaunchKernelGGL(mol_stats_dups, dim3(static_cast<unsigned>(B)), dim3(MST_THREADS), 0, stream, atoms, rows, n_bonds,
                           N, cap, keys, mol);
    }
    hipLaunchKernelGGL(mol_stats_totals, dim3(1), dim3(MST_THREADS), 0, stream, mol, n_bonds, B, cap,
                       reinterpret_cast<long long*>(tot));
    return check_launch("dg_mol_stats");
}
