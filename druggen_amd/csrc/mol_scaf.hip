// Scaffolds and ring systems of the valid molecules of a decoded batch (dg_mol_scaffold of include/druggen_hip_scaf.h, DESIGN
// 3.33): the core (what peeling the atoms of degree <= 1 leaves), the exo atoms double-bonded to it, the scaffold as the fields of
// a second decoded batch, ring systems, and the ring size of every ring bond.  Integers only, no atomics but LDS integer ones
// (exact in any order), every loop carries its trip limit, nothing waits on another workgroup.
//
//   mol_scaf_kernel   one workgroup per molecule, one thread per atom (64..256 threads).  Two sets of bit rows in LDS (mol_ring.h's
//                     row_stride): the BONDS and the RING BONDS.  The bond list stays in global memory and is walked once per
//                     phase -- bit rows, exo atoms, ring sizes, compaction -- so no bond count is refused.  Peeling and the two
//                     min-label propagations (ring systems; the components of the scaffold graph) are synchronous rounds of at
//                     most N, left through one workgroup-wide vote.  The ring size of a ring bond is a breadth-first search over
//                     the ring rows by ONE thread, its frontier and visited sets in registers (2, 4 or 8 words, compile-time
//                     unrolled); the ring bonds are strided over the threads.  The scaffold's rows are compacted in list order by
//                     a ballot prefix per wave and one LDS word per wave, a chunk of blockDim rows at a time.  The sums are
//                     wave64 DPP reductions (lane_reduce.h) added in wave order.  The status is the same in every thread (one
//                     global word), so every branch on it is uniform over the workgroup.
#include "lane_reduce.h"
#include "mol_ring.h"
#include "../../include/druggen_hip_scaf.h"

namespace dg {
namespace {

constexpr int SC_MAX = 256;                                      // atoms, labels, threads
constexpr int SC_WAVES = SC_MAX / 64;
enum { P_A, P_B, P_RING_BONDS, P_COUNT };                        // the packed sums, below

__host__ __device__ constexpr int sc_lds_bytes(int N) { return 2 * N * row_stride(N) * 4; }

// 0 for an UNKNOWN row, else the row's word (mol_valid.hip)
__device__ __forceinline__ unsigned sc_known_bond(unsigned w) {
    const unsigned order = w & 255u;
    const bool bad = order == 0u || order > 3u || (w >> 9) != 0u || ((w >> 8) && order != 1u);
    return bad ? 0u : w;
}

// The table word of row k if it is a BOND of the definition, else 0: both ends below N, different, in the scope, a known label.
__device__ __forceinline__ unsigned sc_bond(unsigned row, unsigned cls, int N, const unsigned char* inscope, const unsigned* btab) {
    const int i = row & 255u, j = (row >> 8) & 255u;
    if (!(cls & DG_DESC_BOND) || i >= N || j >= N || i == j || !inscope[i] || !inscope[j]) return 0u;
    return btab[(row >> 16) & 255u];
}

__device__ __forceinline__ bool sc_bit(const unsigned* words, int a) { return (words[a >> 5] >> (a & 31)) & 1u; }

// Synchronous min-label propagation with one pointer jump per round (decode_graph.hip): lab[a] = a on entry; an atom with
// `mine` takes the smallest label among itself and the atoms of its row that `mask` admits.  Labels only fall and stay inside
// the atom's component, so the fixed point is the smallest index of the component; plain propagation alone reaches it within
// N - 1 rounds, which bounds the loop.  Called by the whole workgroup; lab is final on return.
__device__ __forceinline__ void sc_min_labels(int N, int S, int W, const unsigned* rows, const unsigned* mask, bool mine, int* lab) {
    const int tid = threadIdx.x;
    for (int round = 0; round < N; ++round) {
        int m = tid;
        if (mine) {
            m = lab[tid];
            for (int w = 0; w < W; ++w) {
                unsigned left = rows[tid * S + w] & mask[w];
                for (int step = 0; step < 32 && left; ++step) {
                    m = min(m, lab[32 * w + __ffs(left) - 1]);
                    left &= left - 1u;
                }
            }
            m = min(m, lab[m]);
        }
        const int changed = __syncthreads_or(mine && m != lab[tid]);      // every read of this round is done
        if (!changed) break;
        if (mine) lab[tid] = m;
        __syncthreads();
    }
}

// 1 + the length of the shortest path from i to j over `rows` that does not use the bond (i, j), saturated; one thread, the sets
// in registers.  WORDS >= W: the words of a row that are read.
template <int WORDS>
__device__ __forceinline__ unsigned sc_ring_size(const unsigned* rows, int S, int W, int N, int i, int j) {
    unsigned front[WORDS], vis[WORDS];
#pragma unroll
    for (int w = 0; w < WORDS; ++w) {
        front[w] = w < W ? rows[i * S + w] : 0u;
        vis[w] = 0u;
        if (w == (i >> 5)) vis[w] = 1u << (i & 31);
        if (w == (j >> 5)) front[w] &= ~(1u << (j & 31));             // not over the bond itself
    }
    for (int level = 1; level < N; ++level) {                       // front: the atoms at distance `level` from i
        unsigned next[WORDS];
#pragma unroll
        for (int w = 0; w < WORDS; ++w) next[w] = 0u;
#pragma unroll
        for (int w = 0; w < WORDS; ++w) {
            unsigned left = front[w];
            vis[w] |= left;
            for (int step = 0; step < 32 && left; ++step) {
                const unsigned* row = rows + (32 * w + __ffs(left) - 1) * S;
                left &= left - 1u;
#pragma unroll
                for (int x = 0; x < WORDS; ++x)
                    if (x < W) next[x] |= row[x];
            }
        }
        unsigned any = 0u, hit = 0u;
#pragma unroll
        for (int w = 0; w < WORDS; ++w) {
            next[w] &= ~vis[w];
            any |= next[w];
            if (w == (j >> 5)) hit = (next[w] >> (j & 31)) & 1u;
            front[w] = next[w];
        }
        if (hit) return min(level + 2, DG_SCAF_MAX_RING);           // a path of level + 1 bonds, and the bond
        if (!any) break;
    }
    return DG_SCAF_MAX_RING;
}

__global__ __launch_bounds__(SC_MAX) void mol_scaf_kernel(
    const unsigned char* __restrict__ atoms, const unsigned* __restrict__ bonds, const int* __restrict__ n_bonds,
    const int* __restrict__ desc, const unsigned* __restrict__ atom_key, const unsigned char* __restrict__ bond_class,
    const unsigned* __restrict__ bond_table, int n_bond_labels, int N, int cap, int* __restrict__ mol, int* __restrict__ ring_hist,
    unsigned char* __restrict__ atom_role, unsigned char* __restrict__ atom_system, unsigned char* __restrict__ bond_ring_size,
    unsigned char* __restrict__ s_atoms, unsigned* __restrict__ s_bonds, int* __restrict__ s_n_bonds,
    unsigned char* __restrict__ s_component, int* __restrict__ s_n_components, int* __restrict__ s_largest,
    int* __restrict__ s_largest_size) {
    extern __shared__ __align__(16) unsigned char dyn[];
    const int S = row_stride(N), W = (N + 31) >> 5;
    unsigned* adj = reinterpret_cast<unsigned*>(dyn);               // adj[v * S + w]: bits 32 w .. 32 w + 31 of atom v's BONDS
    unsigned* radj = adj + N * S;                                   // ... of its RING BONDS
    __shared__ unsigned btab[SC_MAX];                               // the bond table; 0: an UNKNOWN row
    __shared__ int sys[SC_MAX], comp[SC_MAX], sys_size[SC_MAX], comp_size[SC_MAX];
    __shared__ unsigned char inscope[SC_MAX], exo[SC_MAX];
    __shared__ unsigned alive[8], ringw[8], scafw[8];               // the core while it is peeled; the ring atoms; the scaffold
    __shared__ unsigned hist[DG_SCAF_HIST_BINS], part[SC_WAVES][P_COUNT], wsum[SC_WAVES];
    __shared__ int ring_min, ring_max, sys_best, comp_best, n_comp;

    const int tid = threadIdx.x, nt = blockDim.x;                   // nt >= N, whole waves
    const int lane = tid & 63, wv = tid >> 6;
    const int64_t b = blockIdx.x;
    const int rows = max(min(n_bonds[b], cap), 0);
    const unsigned* list = bonds + b * cap;
    const int status = desc[b * DG_DESC_FIELDS];

    if (status != DG_VALID_OK) {                                    // (uniform over the workgroup) the empty result
        if (tid < N) {
            atom_role[b * N + tid] = DG_SCAF_ROLE_NONE;
            atom_system[b * N + tid] = DG_SCAF_NO_SYSTEM;
            s_atoms[b * N + tid] = 0;
            s_component[b * N + tid] = static_cast<unsigned char>(tid);
        }
        for (int k = tid; k < rows; k += nt) bond_ring_size[b * cap + k] = 0;
        if (tid < DG_SCAF_MOL_FIELDS) mol[b * DG_SCAF_MOL_FIELDS + tid] = tid == 0 ? status : 0;
        if (tid < DG_SCAF_HIST_BINS) ring_hist[b * DG_SCAF_HIST_BINS + tid] = 0;
        if (tid == 0) {
            s_n_bonds[b] = 0;
            s_n_components[b] = N;
            s_largest[b] = 0;
            s_largest_size[b] = 1;
        }
        return;
    }

    for (int w = tid; w < 2 * N * S; w += nt) adj[w] = 0u;
    for (int i = tid; i < SC_MAX; i += nt) {
        btab[i] = i < n_bond_labels ? sc_known_bond(bond_table[i]) : 0u;
        inscope[i] = i < N && atom_key[b * N + i] != DG_DESC_NO_KEY;
        exo[i] = 0;
        sys[i] = comp[i] = i;
        sys_size[i] = comp_size[i] = 0;
    }
    if (tid < 8) alive[tid] = ringw[tid] = scafw[tid] = 0u;
    if (tid < DG_SCAF_HIST_BINS) hist[tid] = 0u;
    if (tid == 0) {
        ring_min = DG_SCAF_MAX_RING + 1;
        ring_max = sys_best = comp_best = n_comp = 0;
    }
    __syncthreads();

    // ---- the BONDS and the RING BONDS as bit rows ----
    for (int k = tid; k < rows; k += nt) {
        const unsigned row = list[k], cls = bond_class[b * cap + k];
        if (!sc_bond(row, cls, N, inscope, btab)) continue;
        const int i = row & 255u, j = (row >> 8) & 255u;
        atomicOr(&adj[i * S + (j >> 5)], 1u << (j & 31));
        atomicOr(&adj[j * S + (i >> 5)], 1u << (i & 31));
        if (cls & DG_DESC_RING_BOND) {
            atomicOr(&radj[i * S + (j >> 5)], 1u << (j & 31));
            atomicOr(&radj[j * S + (i >> 5)], 1u << (i & 31));
        }
    }
    const bool in = tid < N && inscope[tid];
    if (in) atomicOr(&alive[tid >> 5], 1u << (tid & 31));
    __syncthreads();

    bool ringed = false;
    if (in)
        for (int w = 0; w < W; ++w) ringed |= radj[tid * S + w] != 0u;
    if (ringed) atomicOr(&ringw[tid >> 5], 1u << (tid & 31));

    // ---- the core: every round drops the atoms with at most one BOND to a remaining atom (a chain of N loses two per round) ----
    bool core = in;
    for (int round = 0; round < N; ++round) {
        bool drop = false;
        if (core) {
            int left = 0;
            for (int w = 0; w < W; ++w) left += __popc(adj[tid * S + w] & alive[w]);
            drop = left <= 1;
        }
        const int changed = __syncthreads_or(drop);                 // every read of this round is done
        if (!changed) break;
        if (drop) {
            atomicAnd(&alive[tid >> 5], ~(1u << (tid & 31)));
            core = false;
        }
        __syncthreads();
    }

    // ---- the exo atoms: outside the core, a double BOND to it ----
    for (int k = tid; k < rows; k += nt) {
        const unsigned row = list[k];
        if (sc_bond(row, bond_class[b * cap + k], N, inscope, btab) != 2u) continue;      // order 2, not aromatic
        const int i = row & 255u, j = (row >> 8) & 255u;
        const bool ci = sc_bit(alive, i), cj = sc_bit(alive, j);
        if (ci != cj) exo[ci ? j : i] = 1;                          // (plain byte stores of one value: any order)
    }
    __syncthreads();
    const bool is_exo = in && exo[tid], scaffold = core || is_exo;
    if (scaffold) atomicOr(&scafw[tid >> 5], 1u << (tid & 31));
    __syncthreads();

    // ---- ring systems over the ring rows; the components of the scaffold graph over the rows of the BONDS ----
    sc_min_labels(N, S, W, radj, ringw, ringed, sys);
    sc_min_labels(N, S, W, adj, scafw, scaffold, comp);
    if (tid < N) {
        if (ringed) atomicAdd(&sys_size[sys[tid]], 1);
        atomicAdd(&comp_size[comp[tid]], 1);
        if (comp[tid] == tid) atomicAdd(&n_comp, 1);
    }
    __syncthreads();
    if (tid < N) {
        if (ringed && sys[tid] == tid) atomicMax(&sys_best, sys_size[tid]);
        if (comp[tid] == tid) atomicMax(&comp_best, comp_size[tid] * 256 + (255 - tid));      // ties: the smaller index
    }

    // ---- the ring size of every ring bond: one search per bond, the bonds strided over the threads ----
    unsigned my_ring_bonds = 0u;
    for (int k = tid; k < rows; k += nt) {
        const unsigned row = list[k], cls = bond_class[b * cap + k];
        unsigned size = 0u;
        if ((cls & DG_DESC_RING_BOND) && sc_bond(row, cls, N, inscope, btab)) {
            const int i = row & 255u, j = (row >> 8) & 255u;
            size = W <= 2 ? sc_ring_size<2>(radj, S, W, N, i, j) : W <= 4 ? sc_ring_size<4>(radj, S, W, N, i, j)
                                                                         : sc_ring_size<8>(radj, S, W, N, i, j);
            ++my_ring_bonds;
            atomicAdd(&hist[size <= 8u ? size - 3u : size <= 12u ? 6u : 7u], 1u);
            atomicMin(&ring_min, static_cast<int>(size));
            atomicMax(&ring_max, static_cast<int>(size));
        }
        bond_ring_size[b * cap + k] = static_cast<unsigned char>(size);
    }

    // ---- the scaffold's rows in list order: a ballot prefix per wave, the waves' totals through LDS, blockDim rows per turn ----
    unsigned kept = 0u;                                             // the rows written so far (the same in every thread)
    unsigned* out_rows = s_bonds + b * cap;
    for (int base = 0; base < rows; base += nt) {
        const int k = base + tid;
        unsigned row = 0u;
        bool keep = false;
        if (k < rows) {
            row = list[k];
            keep = sc_bond(row, bond_class[b * cap + k], N, inscope, btab) && sc_bit(scafw, row & 255u) && sc_bit(scafw, (row >> 8) & 255u);
        }
        const unsigned long long votes = __ballot(keep);
        if (lane == 0) wsum[wv] = __popcll(votes);
        __syncthreads();
        unsigned before = kept;
        for (int w = 0; w < SC_WAVES; ++w) {
            const unsigned n = w < (nt >> 6) ? wsum[w] : 0u;
            if (w < wv) before += n;
            kept += n;
        }
        if (keep) out_rows[before + __popcll(votes & ((1ull << lane) - 1ull))] = row & 0x00FFFFFFu;      // (< rows <= cap)
        __syncthreads();                                            // wsum is read before the next turn writes it
    }

    // ---- per atom: role, system, the derived batch's label and component; the sums ----
    unsigned sum_a = 0u, sum_b = 0u;
    if (tid < N) {
        const unsigned role = !in ? DG_SCAF_ROLE_NONE : ringed ? DG_SCAF_ROLE_RING : core ? DG_SCAF_ROLE_LINKER
                                  : is_exo ? DG_SCAF_ROLE_EXO : DG_SCAF_ROLE_SIDE;
        atom_role[b * N + tid] = static_cast<unsigned char>(role);
        atom_system[b * N + tid] = static_cast<unsigned char>(ringed ? sys[tid] : DG_SCAF_NO_SYSTEM);
        s_atoms[b * N + tid] = scaffold ? atoms[b * N + tid] : static_cast<unsigned char>(0);
        s_component[b * N + tid] = static_cast<unsigned char>(comp[tid]);
        sum_a = (in ? 1u : 0u) | (scaffold ? 1u << 10 : 0u) | (is_exo ? 1u << 20 : 0u);      // heavy, scaffold, exo
        sum_b = (core && !ringed ? 1u : 0u) | (ringed ? 1u << 10 : 0u) | (ringed && sys[tid] == tid ? 1u << 20 : 0u);      // linker, ring atoms, systems
    }
    sum_a = wave_usum(sum_a);
    sum_b = wave_usum(sum_b);
    my_ring_bonds = wave_usum(my_ring_bonds);
    if (lane == 0) {
        unsigned* mine = part[wv];
        mine[P_A] = sum_a;
        mine[P_B] = sum_b;
        mine[P_RING_BONDS] = my_ring_bonds;
    }
    __syncthreads();                                                // ... and hist, ring_min / ring_max, the best keys are final
    if (tid < DG_SCAF_MOL_FIELDS) {
        unsigned tot[P_COUNT] = {0u, 0u, 0u};
        for (int w = 0; w < nt >> 6; ++w)
            for (int k = 0; k < P_COUNT; ++k) tot[k] += part[w][k];
        const unsigned ring_atoms = (tot[P_B] >> 10) & 1023u, systems = tot[P_B] >> 20, ring_bonds = tot[P_RING_BONDS];
        unsigned v = 0u;
        if (tid == 0) v = static_cast<unsigned>(status);
        else if (tid == 1) v = tot[P_A] & 1023u;
        else if (tid == 2) v = (tot[P_A] >> 10) & 1023u;
        else if (tid == 3) v = kept;
        else if (tid == 4) v = tot[P_A] >> 20;
        else if (tid == 5) v = tot[P_B] & 1023u;
        else if (tid == 6) v = ring_atoms;
        else if (tid == 7) v = ring_bonds;
        else if (tid == 8) v = ring_bonds - ring_atoms + systems;
        else if (tid == 9) v = systems;
        else if (tid == 10) v = static_cast<unsigned>(sys_best);
        else if (tid == 11) v = ring_bonds ? static_cast<unsigned>(ring_min) : 0u;
        else if (tid == 12) v = static_cast<unsigned>(ring_max);
        mol[b * DG_SCAF_MOL_FIELDS + tid] = static_cast<int>(v);
    }
    if (tid < DG_SCAF_HIST_BINS) ring_hist[b * DG_SCAF_HIST_BINS + tid] = static_cast<int>(hist[tid]);
    if (tid == 0) {
        s_n_bonds[b] = static_cast<int>(kept);
        s_n_components[b] = n_comp;
        s_largest[b] = 255 - (comp_best & 255);
        s_largest_size[b] = comp_best >> 8;
    }
}

}  // namespace
}  // namespace dg

using namespace dg;

extern "C" int dg_mol_scaffold(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds, const int* desc,
                               const unsigned* atom_key, const unsigned char* bond_class, const unsigned* bond_table,
                               int n_bond_labels, int B, int N, int cap, int* mol, int* ring_hist, unsigned char* atom_role,
                               unsigned char* atom_system, unsigned char* bond_ring_size, unsigned char* s_atoms,
                               unsigned char* s_bonds, int* s_n_bonds, unsigned char* s_component, int* s_n_components,
                               int* s_largest, int* s_largest_size, dg_stream_t stream_) {
    if (B < 0 || N < 1 || N > 256 || cap < 0 || n_bond_labels < 1 || n_bond_labels > 256)
        return fail(DG_E_SHAPE, "dg_mol_scaffold: need B >= 0, 1 <= N <= 256, cap >= 0, 1 <= n_bond_labels <= 256 (B=%d N=%d cap=%d "
                    "n_bond_labels=%d)", B, N, cap, n_bond_labels);
    if (!atoms || !n_bonds || !desc || !atom_key || !bond_table || !mol || !ring_hist || !atom_role || !atom_system || !s_atoms ||
        !s_n_bonds || !s_component || !s_n_components || !s_largest || !s_largest_size)
        return fail(DG_E_ARG, "dg_mol_scaffold: null pointer");
    if (cap > 0 && (!bonds || !bond_class || !bond_ring_size || !s_bonds))
        return fail(DG_E_ARG, "dg_mol_scaffold: null pointer (bonds / bond_class / bond_ring_size / s_bonds with cap > 0)");
    if (misaligned(bonds, 4) || misaligned(n_bonds, 4) || misaligned(desc, 4) || misaligned(atom_key, 4) || misaligned(bond_table, 4) ||
        misaligned(mol, 4) || misaligned(ring_hist, 4) || misaligned(s_bonds, 4) || misaligned(s_n_bonds, 4) ||
        misaligned(s_n_components, 4) || misaligned(s_largest, 4) || misaligned(s_largest_size, 4))
        return fail(DG_E_ARG, "dg_mol_scaffold: bond rows of both batches, the table, int arrays, desc and atom_key must be 4-byte aligned");
    if (B == 0) return 0;
    const int threads = max(64, (N + 63) & ~63);                    // one thread per atom, whole waves
    hipLaunchKernelGGL(mol_scaf_kernel, dim3(static_cast<unsigned>(B)), dim3(threads), static_cast<size_t>(sc_lds_bytes(N)),
                       static_cast<hipStream_t>(stream_), atoms, reinterpret_cast<const unsigned*>(bonds), n_bonds, desc, atom_key,
                       bond_class, bond_table, n_bond_labels, N, cap, mol, ring_hist, atom_role, atom_system, bond_ring_size, s_atoms,
                       reinterpret_cast<unsigned*>(s_bonds), s_n_bonds, s_component, s_n_components, s_largest, s_largest_size);
    return check_launch("dg_mol_scaffold");
}
