// Descriptors of the valid molecules of a decoded batch (dg_mol_descriptors of include/druggen_hip_desc.h):
// rotatable bonds, a table-driven polar surface area, ring and carbon counts, and the environment key of every atom.  Integers
// only, no atomics but LDS integer ones (exact in any order), every loop carries its trip limit, nothing waits on another
// workgroup.
//
//   mol_desc_kernel   one workgroup per molecule, one thread per atom (64..256 threads).  The bond list stays in global memory
//                     and is walked once per phase -- scope, bond counts and bit rows, bridges (mol_ring.h), bond classes --
//                     so no bond count is refused.  The per-atom part (triangle test over the bit rows, key, binary search of
//                     env_table: mol_env.h) is one thread per atom; the sums are wave64 DPP reductions (lane_reduce.h) that
//                     meet through one LDS word per wave, added in wave order.  The status is the same in every thread (one
//                     global word and the launch's own arguments), so every branch on it is uniform over the workgroup.
#include "lane_reduce.h"
#include "mol_env.h"
#include "mol_ring.h"
#include "../../include/druggen_hip_desc.h"

namespace dg {
namespace {

constexpr int MD_MAX = 256;                                      // atoms, labels, threads
constexpr int MD_WAVES = MD_MAX / 64;
enum { S_A, S_B, S_C, S_TPSA, S_BONDS, S_COUNT };                // the packed sums, below

__host__ __device__ constexpr int md_lds_bytes(int N) { return N * row_stride(N) * 4; }

// 0 for an UNKNOWN row, else the row's word (mol_valid.hip)
__device__ __forceinline__ unsigned md_known_bond(unsigned w) {
    const unsigned order = w & 255u;
    const bool bad = order == 0u || order > 3u || (w >> 9) != 0u || ((w >> 8) && order != 1u);
    return bad ? 0u : w;
}
// which byte of cnt[] a bond of table word w counts in: 0 single, 1 double, 2 triple, 3 aromatic
__device__ __forceinline__ int md_kind(unsigned w) { return (w >> 8) ? 3 : static_cast<int>(w & 255u) - 1; }

__global__ __launch_bounds__(MD_MAX) void mol_desc_kernel(
    const unsigned char* __restrict__ atoms, const unsigned* __restrict__ bonds, const int* __restrict__ n_bonds,
    const unsigned char* __restrict__ component, const int* __restrict__ largest, const int* __restrict__ flags,
    const int* __restrict__ mol, const unsigned char* __restrict__ hcount, const unsigned* __restrict__ bond_table,
    int n_bond_labels, const unsigned* __restrict__ atom_flags, const unsigned* __restrict__ atom_class, int n_atom_labels,
    const unsigned* __restrict__ env_table, int n_env, int N, int cap, int scope, int* __restrict__ desc,
    unsigned* __restrict__ atom_key, unsigned char* __restrict__ bond_class) {
    extern __shared__ __align__(16) unsigned char dyn[];
    const int S = row_stride(N), W = (N + 31) >> 5;
    unsigned* adj = reinterpret_cast<unsigned*>(dyn);               // adj[v * S + w]: bits 32 w .. 32 w + 31 of atom v's row
    __shared__ unsigned btab[MD_MAX];                               // the bond table; 0: an UNKNOWN row
    __shared__ unsigned cnt[MD_MAX], deg[MD_MAX];                   // cnt: n1 | n2 << 8 | n3 << 16 | na << 24
    __shared__ unsigned short parent[MD_MAX], depth[MD_MAX];        // the breadth-first forest
    __shared__ unsigned char lab_a[MD_MAX], member[MD_MAX], cov[MD_MAX], ringed[MD_MAX];
    __shared__ unsigned front[8], vis[8], bonded[8];
    __shared__ unsigned part[MD_WAVES][S_COUNT];

    const int tid = threadIdx.x, nt = blockDim.x;                   // nt >= N, whole waves
    const int64_t b = blockIdx.x;
    const int nb = n_bonds[b];
    const int rows = max(min(nb, cap), 0);                          // the entries of bond_class this call stores
    const unsigned* list = bonds + b * cap;
    const int status = (nb > cap || (flags && flags[b] < 0)) ? DG_VALID_NO_GRAPH : mol[b * DG_VALID_MOL_FIELDS];

    if (status != DG_VALID_OK) {                                    // (uniform over the workgroup)
        if (tid < N) atom_key[b * N + tid] = DG_DESC_NO_KEY;
        for (int k = tid; k < rows; k += nt) bond_class[b * cap + k] = 0;
        if (tid < DG_DESC_FIELDS) desc[b * DG_DESC_FIELDS + tid] = tid == 0 ? status : 0;
        return;
    }

    for (int w = tid; w < N * S; w += nt) adj[w] = 0u;
    for (int i = tid; i < MD_MAX; i += nt) {
        cnt[i] = deg[i] = 0u;
        parent[i] = RING_NONE;
        depth[i] = 0;
        member[i] = cov[i] = ringed[i] = 0;
        lab_a[i] = i < N ? atoms[b * N + i] : 0;
        btab[i] = i < n_bond_labels ? md_known_bond(bond_table[i]) : 0u;
    }
    if (tid < 8) front[tid] = vis[tid] = bonded[tid] = 0u;
    __syncthreads();

    // ---- the scope ----
    if (scope == DG_CANON_WHOLE) {
        for (int k = tid; k < rows; k += nt) {
            const unsigned row = list[k];
            const int i = row & 255u, j = (row >> 8) & 255u;
            if (i < N && j < N && i != j) member[i] = member[j] = 1;      // (plain byte stores of one value: any order)
        }
        __syncthreads();
        for (int i = tid; i < N; i += nt) member[i] = member[i] || lab_a[i] != 0;
    } else {
        const int root = largest[b];
        for (int i = tid; i < N; i += nt) member[i] = component[b * N + i] == root;
    }
    __syncthreads();

    // ---- the BONDS: counts by kind, degrees, bit rows ----
    unsigned my_bonds = 0u;
    for (int k = tid; k < rows; k += nt) {
        const unsigned row = list[k];
        const int i = row & 255u, j = (row >> 8) & 255u;
        if (i >= N || j >= N || i == j || !member[i] || !member[j]) continue;
        ++my_bonds;
        const unsigned w = btab[(row >> 16) & 255u];
        atomicAdd(&deg[i], 1u);
        atomicAdd(&deg[j], 1u);
        if (w) {                                                    // (a valid molecule has no UNKNOWN bond)
            const unsigned one = 1u << (8 * md_kind(w));
            atomicAdd(&cnt[i], one);
            atomicAdd(&cnt[j], one);
        }
        atomicOr(&adj[i * S + (j >> 5)], 1u << (j & 31));
        atomicOr(&adj[j * S + (i >> 5)], 1u << (i & 31));
    }
    __syncthreads();
    if (tid < N && deg[tid]) atomicOr(&bonded[tid >> 5], 1u << (tid & 31));

    // ---- bridges (mol_ring.h): a breadth-first forest, then the tree paths that the bonds outside it close ----
    ring_forest(N, adj, deg, bonded, front, vis, parent, depth);
    ring_cover(N, list, rows, member, parent, depth, cov, nullptr);
    __syncthreads();

    // ---- the class of every row; the atoms with a ring bond ----
    unsigned my_rot = 0u;
    for (int k = tid; k < rows; k += nt) {
        const unsigned row = list[k];
        const int i = row & 255u, j = (row >> 8) & 255u;
        unsigned cls = 0u;
        if (i < N && j < N && i != j && member[i] && member[j]) {
            const int child = parent[i] == j ? i : parent[j] == i ? j : -1;      // a tree bond hangs below its child
            const bool bridge = child >= 0 && !cov[child];
            const unsigned w = btab[(row >> 16) & 255u];
            const bool rot = bridge && w == 1u && deg[i] >= 2u && deg[j] >= 2u && !((cnt[i] | cnt[j]) & 0x00FF0000u);
            cls = DG_DESC_BOND | (bridge ? 0u : DG_DESC_RING_BOND) | (rot ? DG_DESC_ROTATABLE : 0u);
            if (!bridge) ringed[i] = ringed[j] = 1;                 // (as above, and as mol_ring.h marks cov)
            my_rot += rot;
        }
        bond_class[b * cap + k] = static_cast<unsigned char>(cls);
    }
    __syncthreads();

    // ---- per atom: the triangle test, the key, its row of env_table ----
    unsigned sum_a = 0u, sum_b = 0u, sum_c = my_rot << 10, tpsa = 0u, key = DG_DESC_NO_KEY;
    if (tid < N && member[tid]) {
        const unsigned c = cnt[tid], n1 = c & 255u, n2 = (c >> 8) & 255u, n3 = (c >> 16) & 255u, na = c >> 24;
        const unsigned lab = lab_a[tid];
        const unsigned* mine = adj + tid * S;
        unsigned r3 = 0u;
        for (int w = 0; w < W; ++w) {
            unsigned left = mine[w];
            for (int step = 0; step < 32 && left; ++step) {         // every neighbour: does its row meet mine?
                const unsigned* other = adj + (32 * w + __ffs(left) - 1) * S;
                left &= left - 1u;
                for (int x = 0; x < W; ++x) r3 |= mine[x] & other[x];
            }
        }
        r3 = r3 != 0u;
        key = env_key(lab, hcount[b * N + tid], n1, n2, n3, na, r3);
        const int at = env_find(env_table, n_env, key);             // one thread per atom, the table from L2
        const bool typed = at >= 0;
        if (typed) tpsa = env_table[4 * at + 1];
        const bool known = lab < static_cast<unsigned>(n_atom_labels);
        const bool polar = known && (atom_flags[lab] & 1u), carbon = known && (atom_class[lab] & 1u);
        sum_a = 1u | (parent[tid] == RING_NONE ? 1u << 10 : 0u) | (ringed[tid] ? 1u << 20 : 0u);      // atoms, components, ring atoms
        sum_b = (na ? 1u : 0u) | (carbon ? 1u << 10 : 0u) | (carbon && !(c >> 8) ? 1u << 20 : 0u);     // aromatic, carbon, sp3 carbon
        sum_c += polar && !typed;                                                                     // untyped | n_rot << 10
    }
    if (tid < N) atom_key[b * N + tid] = key;

    // ---- the sums: at most 256 per 10-bit field, at most 32640 BONDS ----
    sum_a = wave_usum(sum_a);
    sum_b = wave_usum(sum_b);
    sum_c = wave_usum(sum_c);
    tpsa = wave_usum(tpsa);
    my_bonds = wave_usum(my_bonds);
    if ((tid & 63) == 0) {
        unsigned* mine = part[tid >> 6];
        mine[S_A] = sum_a;
        mine[S_B] = sum_b;
        mine[S_C] = sum_c;
        mine[S_TPSA] = tpsa;
        mine[S_BONDS] = my_bonds;
    }
    __syncthreads();
    if (tid < DG_DESC_FIELDS) {
        unsigned tot[S_COUNT] = {0u, 0u, 0u, 0u, 0u};
        for (int w = 0; w < nt >> 6; ++w)
            for (int k = 0; k < S_COUNT; ++k) tot[k] += part[w][k];
        const unsigned heavy = tot[S_A] & 1023u, comps = (tot[S_A] >> 10) & 1023u;
        unsigned v = 0u;
        if (tid == 0) v = static_cast<unsigned>(status);
        else if (tid == 1) v = heavy;
        else if (tid == 2) v = tot[S_C] >> 10;
        else if (tid == 3) v = tot[S_TPSA];
        else if (tid == 4) v = tot[S_C] & 1023u;
        else if (tid == 5) v = tot[S_BONDS] - heavy + comps;
        else if (tid == 6) v = tot[S_A] >> 20;
        else if (tid == 7) v = tot[S_B] & 1023u;
        else if (tid == 8) v = (tot[S_B] >> 10) & 1023u;
        else if (tid == 9) v = tot[S_B] >> 20;
        desc[b * DG_DESC_FIELDS + tid] = static_cast<int>(v);
    }
}

}  // namespace
}  // namespace dg

using namespace dg;

extern "C" int dg_mol_descriptors(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds,
                                  const unsigned char* component, const int* largest, const int* flags, const int* mol,
                                  const unsigned char* hcount, const unsigned* bond_table, int n_bond_labels,
                                  const unsigned* atom_flags, const unsigned* atom_class, int n_atom_labels,
                                  const unsigned* env_table, int n_env, int B, int N, int cap, int scope, int* desc,
                                  unsigned* atom_key, unsigned char* bond_class, dg_stream_t stream_) {
    if (B < 0 || N < 1 || N > 256 || cap < 0 || n_atom_labels < 1 || n_atom_labels > 255 || n_bond_labels < 1 ||
        n_bond_labels > 256 || n_env < 0 || n_env > DG_DESC_MAX_ENV)
        return fail(DG_E_SHAPE, "dg_mol_descriptors: need B >= 0, 1 <= N <= 256, cap >= 0, 1 <= n_atom_labels <= 255, "
                    "1 <= n_bond_labels <= 256, 0 <= n_env <= %d (B=%d N=%d cap=%d n_atom_labels=%d n_bond_labels=%d n_env=%d)",
                    DG_DESC_MAX_ENV, B, N, cap, n_atom_labels, n_bond_labels, n_env);
    if (scope != DG_CANON_WHOLE && scope != DG_CANON_LARGEST)
        return fail(DG_E_ARG, "dg_mol_descriptors: scope must be 0 (whole) or 1 (largest), got %d", scope);
    if (!atoms || !n_bonds || !mol || !hcount || !bond_table || !atom_flags || !atom_class || !desc || !atom_key)
        return fail(DG_E_ARG, "dg_mol_descriptors: null pointer");
    if (scope == DG_CANON_LARGEST && (!component || !largest))
        return fail(DG_E_ARG, "dg_mol_descriptors: null pointer (component / largest with scope 1)");
    if (cap > 0 && (!bonds || !bond_class)) return fail(DG_E_ARG, "dg_mol_descriptors: null pointer (bonds / bond_class with cap > 0)");
    if (n_env > 0 && !env_table) return fail(DG_E_ARG, "dg_mol_descriptors: null pointer (env_table with n_env > 0)");
    if (misaligned(bonds, 4) || misaligned(n_bonds, 4) || misaligned(largest, 4) || misaligned(flags, 4) || misaligned(mol, 4) ||
        misaligned(bond_table, 4) || misaligned(atom_flags, 4) || misaligned(atom_class, 4) || misaligned(env_table, 4) ||
        misaligned(desc, 4) || misaligned(atom_key, 4))
        return fail(DG_E_ARG, "dg_mol_descriptors: bond rows, tables, int arrays, desc and atom_key must be 4-byte aligned");
    if (B == 0) return 0;
    const int threads = max(64, (N + 63) & ~63);                    // one thread per atom, whole waves
    hipLaunchKernelGGL(mol_desc_kernel, dim3(static_cast<unsigned>(B)), dim3(threads), static_cast<size_t>(md_lds_bytes(N)),
                       static_cast<hipStream_t>(stream_), atoms, reinterpret_cast<const unsigned*>(bonds), n_bonds, component,
                       largest, flags, mol, hcount, bond_table, n_bond_labels, atom_flags, atom_class, n_atom_labels, env_table,
                       n_env, N, cap, scope, desc, atom_key, bond_class);
    return check_launch("dg_mol_descriptors");
}
