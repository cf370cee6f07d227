// Validity of a decoded batch (dg_mol_validity of include/druggen_hip_valid.h): allowed valences, aromatic bonds
// in rings, a Kekule structure, and from it hydrogens, mass and polar atoms.  Integers only, no atomics but LDS integer ones
// (exact in any order), every loop carries its trip limit, nothing waits on another workgroup.
//
//   mol_valid_kernel   one workgroup per molecule, one thread per atom (64..256 threads).  The bond list stays in global memory
//                      and is walked once per phase -- scope, valences, bridges and the aromatic graph, the Kekule rows -- so
//                      no bond count is refused.  The phases are parallel but one: the maximum matching of the aromatic graph
//                      (mol_match.h) is run by lane 0 over adjacency lists of at most 7 neighbours in LDS.  The status is
//                      read from LDS after a barrier, so every branch on it is uniform over the workgroup.
#include "mol_match.h"
#include "mol_ring.h"
#include "../../include/druggen_hip_valid.h"

namespace dg {
namespace {

constexpr int MV_MAX = 256;                                      // atoms, labels, threads
constexpr unsigned MV_OVER = 0xFF;                               // w0 of an over-valent atom
enum { T_ATOMS, T_UNKNOWN, T_OVER, T_BRIDGE, T_H, T_MASS, T_DONORS, T_ACCEPTORS, T_FREE, T_COUNT };

__host__ __device__ constexpr int lds_bytes(int N) { return N * row_stride(N) * 4; }

// 0 for an UNKNOWN row, else the row's word
__device__ __forceinline__ unsigned known_valences(unsigned v) {
    const bool bad = (v & 255u) == 0u || (v & 255u) > 8u || ((v >> 8) & 255u) > 8u || ((v >> 16) & 255u) > 8u || (v >> 24) > 8u;
    return bad ? 0u : v;
}
__device__ __forceinline__ unsigned known_bond(unsigned w) {
    const unsigned order = w & 255u;
    const bool bad = order == 0u || order > 3u || (w >> 9) != 0u || ((w >> 8) && order != 1u);
    return bad ? 0u : w;
}

__global__ __launch_bounds__(MV_MAX) void mol_valid_kernel(
    const unsigned char* __restrict__ atoms, const unsigned* __restrict__ bonds, const int* __restrict__ n_bonds,
    const unsigned char* __restrict__ component, const int* __restrict__ largest, const int* __restrict__ flags,
    const unsigned* __restrict__ atom_table, int n_atom_labels, const unsigned* __restrict__ bond_table, int n_bond_labels, int N,
    int cap, int scope, int h_mass, int* __restrict__ mol, unsigned char* __restrict__ hcount, unsigned* __restrict__ kekule) {
    extern __shared__ __align__(16) unsigned char dyn[];
    const int S = row_stride(N);
    unsigned* adj = reinterpret_cast<unsigned*>(dyn);               // adj[v * S + w]: bits 32 w .. 32 w + 31 of atom v's row
    __shared__ unsigned vals[MV_MAX], amass[MV_MAX], btab[MV_MAX];  // the tables; 0: an UNKNOWN row
    __shared__ unsigned sigma[MV_MAX], arom[MV_MAX], deg[MV_MAX], gdeg[MV_MAX], seen[MV_MAX];
    __shared__ unsigned short parent[MV_MAX], depth[MV_MAX];        // the breadth-first forest
    __shared__ unsigned short match[MV_MAX], par[MV_MAX], base[MV_MAX], queue[MV_MAX];      // the matching
    __shared__ unsigned char lab_a[MV_MAX], member[MV_MAX], cov[MV_MAX], cand[MV_MAX], w0[MV_MAX], polar[MV_MAX], used[MV_MAX];
    __shared__ unsigned char gn[MV_MAX * MATCH_DEG];                // gn[a * 7 + k]: the k-th neighbour of a in G
    __shared__ unsigned front[8], vis[8], bonded[8];
    __shared__ int tot[T_COUNT];

    const int tid = threadIdx.x, nt = blockDim.x;                   // nt >= N
    const int64_t b = blockIdx.x;
    const int nb = n_bonds[b];
    const int rows = max(min(nb, cap), 0);                          // the rows of kekule this call stores
    const unsigned* list = bonds + b * cap;
    int status = (nb > cap || (flags && flags[b] < 0)) ? DG_VALID_NO_GRAPH : DG_VALID_OK;      // (uniform over the workgroup)
    const int kept = status == DG_VALID_OK ? rows : 0;

    for (int w = tid; w < N * S; w += nt) adj[w] = 0u;
    for (int i = tid; i < MV_MAX; i += nt) {
        sigma[i] = arom[i] = deg[i] = gdeg[i] = seen[i] = 0u;
        parent[i] = RING_NONE;
        depth[i] = 0;
        match[i] = par[i] = MATCH_NONE;
        base[i] = static_cast<unsigned short>(i);
        member[i] = cov[i] = cand[i] = used[i] = 0;
        w0[i] = MV_OVER;
        lab_a[i] = i < N ? atoms[b * N + i] : 0;
        vals[i] = i < n_atom_labels ? known_valences(atom_table[4 * i]) : 0u;
        amass[i] = i < n_atom_labels ? atom_table[4 * i + 1] : 0u;
        polar[i] = i < n_atom_labels ? atom_table[4 * i + 2] & 1u : 0u;
        btab[i] = i < n_bond_labels ? known_bond(bond_table[i]) : 0u;
    }
    if (tid < 8) front[tid] = vis[tid] = bonded[tid] = 0u;
    if (tid < T_COUNT) tot[tid] = 0;
    __syncthreads();

    if (status == DG_VALID_OK) {
        // ---- the scope ----
        if (scope == DG_CANON_WHOLE) {
            for (int k = tid; k < kept; k += nt) {
                const unsigned row = list[k];
                const int i = row & 255u, j = (row >> 8) & 255u;
                if (i < N && j < N && i != j) member[i] = member[j] = 1;
            }
            __syncthreads();
            for (int i = tid; i < N; i += nt) member[i] = member[i] || lab_a[i] != 0;
        } else {
            const int root = largest[b];
            for (int i = tid; i < N; i += nt) member[i] = component[b * N + i] == root;
        }
        __syncthreads();

        // ---- the bonds inside it: sigma, arom, degrees, bit rows; unknown labels ----
        if (tid < N && member[tid]) {
            atomicAdd(&tot[T_ATOMS], 1);
            if (!vals[lab_a[tid]]) tot[T_UNKNOWN] = 1;
        }
        for (int k = tid; k < kept; k += nt) {
            const unsigned row = list[k];
            const int i = row & 255u, j = (row >> 8) & 255u;
            if (i >= N || j >= N || i == j || !member[i] || !member[j]) continue;
            const unsigned w = btab[(row >> 16) & 255u];
            if (!w) {
                tot[T_UNKNOWN] = 1;
                continue;
            }
            atomicAdd(&deg[i], 1u);
            atomicAdd(&deg[j], 1u);
            atomicAdd(&sigma[i], w & 255u);
            atomicAdd(&sigma[j], w & 255u);
            atomicAdd(&arom[i], w >> 8);
            atomicAdd(&arom[j], w >> 8);
            atomicOr(&adj[i * S + (j >> 5)], 1u << (j & 31));
            atomicOr(&adj[j * S + (i >> 5)], 1u << (i & 31));
        }
        __syncthreads();
        status = tot[T_ATOMS] == 0 ? DG_VALID_EMPTY : tot[T_UNKNOWN] ? DG_VALID_UNKNOWN_LABEL : DG_VALID_OK;
    }

    if (status == DG_VALID_OK) {
        // ---- w0, the over-valent atoms, the candidates ----
        if (tid < N && member[tid]) {
            const unsigned v = vals[lab_a[tid]], s = sigma[tid];
            unsigned best = MV_OVER;
            for (int k = 0; k < 4; ++k) {
                const unsigned allowed = (v >> (8 * k)) & 255u;
                if (!allowed) break;
                if (allowed >= s && allowed < best) best = allowed;
            }
            w0[tid] = static_cast<unsigned char>(best);
            if (best == MV_OVER) atomicAdd(&tot[T_OVER], 1);
            cand[tid] = best != MV_OVER && arom[tid] > 0u && best > s;
            if (deg[tid]) atomicOr(&bonded[tid >> 5], 1u << (tid & 31));
        }
        // ---- bridges (mol_ring.h): a breadth-first forest, then the tree paths that the bonds outside it close ----
        ring_forest(N, adj, deg, bonded, front, vis, parent, depth);
        ring_cover(N, list, kept, member, parent, depth, cov, nullptr);
        __syncthreads();
        // ---- aromatic bonds: none may be a bridge; those between two candidates are the edges of G ----
        for (int k = tid; k < kept; k += nt) {
            const unsigned row = list[k];
            const int i = row & 255u, j = (row >> 8) & 255u;
            if (i >= N || j >= N || i == j || !member[i] || !member[j] || !(btab[(row >> 16) & 255u] >> 8)) continue;
            const int child = parent[i] == j ? i : parent[j] == i ? j : -1;      // a tree bond hangs below its child
            if (child >= 0 && !cov[child]) tot[T_BRIDGE] = 1;
            if (!cand[i] || !cand[j]) continue;
            const unsigned si = atomicAdd(&gdeg[i], 1u), sj = atomicAdd(&gdeg[j], 1u);
            if (si < MATCH_DEG) gn[i * MATCH_DEG + si] = static_cast<unsigned char>(j);      // (arom < w0 <= 8: always)
            if (sj < MATCH_DEG) gn[j * MATCH_DEG + sj] = static_cast<unsigned char>(i);
        }
        __syncthreads();
        status = tot[T_OVER] ? DG_VALID_OVER_VALENT : tot[T_BRIDGE] ? DG_VALID_AROMATIC_NOT_IN_RING : DG_VALID_OK;
    }

    int deficiency = -1;
    if (status == DG_VALID_OK) {
        // ---- the neighbours in ascending order: the slots above were taken in any order, the matching must not depend on it ----
        if (tid < N && cand[tid]) {
            const int d = min(gdeg[tid], static_cast<unsigned>(MATCH_DEG));
            unsigned char* mine = gn + tid * MATCH_DEG;
            for (int x = 1; x < d; ++x) {
                const unsigned char key = mine[x];
                int y = x - 1;
                for (; y >= 0 && mine[y] > key; --y) mine[y + 1] = mine[y];
                mine[y + 1] = key;
            }
        }
        __syncthreads();
        // ---- a maximum matching of G, by one lane ----
        if (tid == 0) {
            MatchState s{match, par, base, queue, used, seen, cand, gn, gdeg, 0u, N, 0};
            tot[T_FREE] = match_maximum(s);
        }
        __syncthreads();
        deficiency = tot[T_FREE];
        if (deficiency) status = DG_VALID_NOT_KEKULISABLE;
    }

    // ---- hydrogens, mass, polar atoms ----
    unsigned h = 0xFFu;
    if (status == DG_VALID_OK && tid < N && member[tid]) {
        h = w0[tid] - sigma[tid] - cand[tid];
        const unsigned char lab = lab_a[tid];
        atomicAdd(&tot[T_H], static_cast<int>(h));
        atomicAdd(&tot[T_MASS], static_cast<int>(amass[lab]));      // (modulo 2^32)
        if (polar[lab]) {
            atomicAdd(&tot[T_ACCEPTORS], 1);
            if (h) atomicAdd(&tot[T_DONORS], 1);
        }
    }
    if (tid < N) hcount[b * N + tid] = static_cast<unsigned char>(h);
    // ---- the Kekule rows ----
    for (int k = tid; k < rows; k += nt) {
        const unsigned row = list[k] & 0x00FFFFFFu;
        const int i = row & 255u, j = (row >> 8) & 255u;
        unsigned order = 0u;
        if (status == DG_VALID_OK && i < N && j < N && i != j && member[i] && member[j]) {
            const unsigned w = btab[(row >> 16) & 255u];
            order = (w >> 8) ? (cand[i] && cand[j] && match[i] == j ? 2u : 1u) : (w & 255u);
        }
        kekule[b * cap + k] = row | order << 24;
    }
    __syncthreads();
    if (tid < DG_VALID_MOL_FIELDS) {
        const bool counted = status != DG_VALID_NO_GRAPH && status != DG_VALID_EMPTY && status != DG_VALID_UNKNOWN_LABEL;
        int v = 0;
        if (tid == 0) v = status;
        else if (tid == 1) v = status == DG_VALID_NO_GRAPH ? 0 : tot[T_ATOMS];
        else if (tid == 2) v = counted ? tot[T_OVER] : 0;
        else if (tid == 3) v = deficiency;
        else if (status == DG_VALID_OK) {
            v = tid == 4 ? tot[T_H] : tid == 6 ? tot[T_DONORS] : tid == 7 ? tot[T_ACCEPTORS]
                : static_cast<int>(static_cast<unsigned>(tot[T_MASS]) + static_cast<unsigned>(tot[T_H]) * static_cast<unsigned>(h_mass));
        }
        mol[b * DG_VALID_MOL_FIELDS + tid] = v;
    }
}

}  // namespace
}  // namespace dg

using namespace dg;

extern "C" int dg_mol_validity(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds,
                               const unsigned char* component, const int* largest, const int* flags, const unsigned* atom_table,
                               int n_atom_labels, const unsigned* bond_table, int n_bond_labels, int B, int N, int cap, int scope,
                               int h_mass, int* mol, unsigned char* hcount, unsigned char* kekule, dg_stream_t stream_) {
    if (B < 0 || N < 1 || N > 256 || cap < 0 || n_atom_labels < 1 || n_atom_labels > 255 || n_bond_labels < 1 || n_bond_labels > 256)
        return fail(DG_E_SHAPE, "dg_mol_validity: need B >= 0, 1 <= N <= 256, cap >= 0, 1 <= n_atom_labels <= 255, "
                    "1 <= n_bond_labels <= 256 (B=%d N=%d cap=%d n_atom_labels=%d n_bond_labels=%d)", B, N, cap, n_atom_labels,
                    n_bond_labels);
    if (scope != DG_CANON_WHOLE && scope != DG_CANON_LARGEST)
        return fail(DG_E_ARG, "dg_mol_validity: scope must be 0 (whole) or 1 (largest), got %d", scope);
    if (h_mass < 0) return fail(DG_E_ARG, "dg_mol_validity: h_mass must be >= 0, got %d", h_mass);
    if (!atoms || !n_bonds || !atom_table || !bond_table || !mol || !hcount) return fail(DG_E_ARG, "dg_mol_validity: null pointer");
    if (scope == DG_CANON_LARGEST && (!component || !largest))
        return fail(DG_E_ARG, "dg_mol_validity: null pointer (component / largest with scope 1)");
    if (cap > 0 && (!bonds || !kekule)) return fail(DG_E_ARG, "dg_mol_validity: null pointer (bonds / kekule with cap > 0)");
    if (misaligned(bonds, 4) || misaligned(n_bonds, 4) || misaligned(largest, 4) || misaligned(flags, 4) ||
        misaligned(atom_table, 4) || misaligned(bond_table, 4) || misaligned(mol, 4) || misaligned(kekule, 4))
        return fail(DG_E_ARG, "dg_mol_validity: bond rows, Kekule rows, tables and int arrays must be 4-byte aligned");
    if (B == 0) return 0;
    const int threads = max(64, (N + 63) & ~63);                    // one thread per atom, whole waves
    hipLaunchKernelGGL(mol_valid_kernel, dim3(static_cast<unsigned>(B)), dim3(threads), static_cast<size_t>(lds_bytes(N)),
                       static_cast<hipStream_t>(stream_), atoms, reinterpret_cast<const unsigned*>(bonds), n_bonds, component,
                       largest, flags, atom_table, n_atom_labels, bond_table, n_bond_labels, N, cap, scope, h_mass, mol, hcount,
                       reinterpret_cast<unsigned*>(kekule));
    return check_launch("dg_mol_validity");
}
