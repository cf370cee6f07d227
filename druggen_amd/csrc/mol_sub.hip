// Substructure patterns on the valid molecules of a decoded batch (dg_mol_substructure of include/druggen_hip_sub.h, DESIGN
// 3.32): per-pattern anchor counts and an ordered first-match atom typing with additive values.  Integers only, no atomics but
// LDS integer ones (exact in any order), every loop carries its trip limit, nothing waits on another workgroup.
//
//   mol_sub_kernel   one workgroup per molecule, 64..256 threads in whole waves.  The molecule is staged in LDS: one property
//                    word and one set word per atom, and per atom at most eight `neighbour << 8 | kind` entries that the
//                    atom's own thread sorts.  The work items are the (pattern, anchor) pairs, pattern-major, strided over
//                    the threads, so that a wave reads one or two pattern records (through L1 / L2: 320 bytes each, the
//                    same for every workgroup) whatever N is.  The search (mol_sub.h) keeps its images and cursors, which a
//                    run-time depth indexes, in LDS -- 32 bytes per thread, interleaved by thread -- not in a private
//                    array.  Results meet through LDS atomicAdd (hits, n_over) and atomicMin (atom_type); the sums are taken
//                    after a barrier, once the types are final, with wave_usum, and added in wave order.  The status is the
//                    same in every thread (one global word), so every branch on it is uniform over the workgroup.
#include "lane_reduce.h"
#include "mol_sub.h"
#include "../../include/druggen_hip_sub.h"

namespace dg {
namespace {

constexpr int MS_MAX = 256;                                      // atoms, threads
constexpr int MS_WAVES = MS_MAX / 64;
constexpr int MS_NONE = 0x7FFFFFFF;                              // no type yet
enum { T_HEAVY, T_TYPED, T_SUM0, T_SUM1, T_HIT, T_COUNT };

static_assert(SUB_MAX_ATOMS == DG_SUB_MAX_ATOMS && SUB_MAX_CLOSURES == DG_SUB_MAX_CLOSURES && SUB_MAX_STEPS == DG_SUB_MAX_STEPS &&
              SUB_NBR == DG_SUB_MAX_NEIGHBOURS && SUB_WORDS == DG_SUB_PATTERN_WORDS, "mol_sub.h and druggen_hip_sub.h disagree");

// 0 for an UNKNOWN row, else the row's word (mol_valid.hip)
__device__ __forceinline__ unsigned ms_known_bond(unsigned w) {
    const unsigned order = w & 255u;
    const bool bad = order == 0u || order > 3u || (w >> 9) != 0u || ((w >> 8) && order != 1u);
    return bad ? 0u : w;
}

__global__ __launch_bounds__(MS_MAX) void mol_sub_kernel(
    const unsigned char* __restrict__ atoms, const unsigned* __restrict__ bonds, const int* __restrict__ n_bonds,
    const int* __restrict__ desc, const unsigned* __restrict__ atom_key, const unsigned char* __restrict__ bond_class,
    const unsigned* __restrict__ bond_table, int n_bond_labels, const unsigned* __restrict__ atom_sets, int n_atom_labels,
    const unsigned* __restrict__ patterns, int n_patterns, int N, int cap, int* __restrict__ mol, int* __restrict__ hits,
    int* __restrict__ atom_type) {
    __shared__ unsigned prop[MS_MAX], sets[MS_MAX], fill[MS_MAX];    // fill: the neighbours seen, before the cut to eight
    __shared__ unsigned short nbr[MS_MAX * SUB_NBR];
    __shared__ unsigned char ncnt[MS_MAX];
    __shared__ int atype[MS_MAX];
    __shared__ int hit[DG_SUB_MAX_PATTERNS];
    __shared__ unsigned char image[SUB_MAX_ATOMS * MS_MAX], cursor[SUB_MAX_ATOMS * MS_MAX];      // [depth][thread]
    __shared__ unsigned part[MS_WAVES][T_COUNT];
    __shared__ unsigned over;

    const int tid = threadIdx.x, nt = blockDim.x;                   // whole waves
    const int64_t b = blockIdx.x;
    const int status = desc[b * DG_DESC_FIELDS];

    if (status != DG_VALID_OK) {                                    // (uniform over the workgroup)
        for (int i = tid; i < N; i += nt) atom_type[b * N + i] = -1;
        for (int p = tid; p < n_patterns; p += nt) hits[b * n_patterns + p] = 0;
        if (tid < DG_SUB_MOL_FIELDS) mol[b * DG_SUB_MOL_FIELDS + tid] = tid == 0 ? status : 0;
        return;
    }

    // ---- per atom: the property word of its key, its set word ----
    for (int i = tid; i < MS_MAX; i += nt) {
        unsigned p = 0u, s = 0u;
        if (i < N) {
            const unsigned key = atom_key[b * N + i], lab = atoms[b * N + i];
            if (key != DG_DESC_NO_KEY) p = sub_prop(key);
            s = lab < static_cast<unsigned>(n_atom_labels) ? atom_sets[lab] : 0u;
        }
        prop[i] = p;
        sets[i] = s;
        fill[i] = 0u;
        ncnt[i] = 0;
        atype[i] = MS_NONE;
    }
    for (int p = tid; p < n_patterns; p += nt) hit[p] = 0;
    if (tid == 0) over = 0u;
    __syncthreads();

    // ---- the BONDS: neighbour entries in arrival order, the atoms with a ring bond ----
    const int rows = max(min(n_bonds[b], cap), 0);
    const unsigned* list = bonds + b * cap;
    for (int k = tid; k < rows; k += nt) {
        const unsigned cls = bond_class[b * cap + k];
        if (!(cls & DG_DESC_BOND)) continue;
        const unsigned row = list[k];
        const int i = row & 255u, j = (row >> 8) & 255u;
        const unsigned lab = (row >> 16) & 255u;
        if (i >= N || j >= N || i == j || !(prop[i] & prop[j] & SUB_IN_SCOPE)) continue;
        const unsigned w = lab < static_cast<unsigned>(n_bond_labels) ? ms_known_bond(bond_table[lab]) : 0u;
        if (!w) continue;
        const bool ring = cls & DG_DESC_RING_BOND;
        const unsigned kind = ((w >> 8) ? 3u : (w & 255u) - 1u) + (ring ? 4u : 0u);
        const unsigned si = atomicAdd(&fill[i], 1u), sj = atomicAdd(&fill[j], 1u);
        if (si < SUB_NBR) nbr[i * SUB_NBR + si] = static_cast<unsigned short>(j << 8 | kind);
        if (sj < SUB_NBR) nbr[j * SUB_NBR + sj] = static_cast<unsigned short>(i << 8 | kind);
        if (ring) {
            atomicOr(&prop[i], SUB_RINGED);
            atomicOr(&prop[j], SUB_RINGED);
        }
    }
    __syncthreads();

    // ---- every thread sorts its own atoms' entries (at most eight: an insertion sort of at most 28 moves) ----
    for (int i = tid; i < N; i += nt) {
        const int n = min(fill[i], static_cast<unsigned>(SUB_NBR));
        unsigned short* mine = nbr + i * SUB_NBR;
        for (int x = 1; x < n; ++x) {
            const unsigned short e = mine[x];
            int y = x;
            for (; y > 0 && mine[y - 1] > e; --y) mine[y] = mine[y - 1];
            mine[y] = e;
        }
        ncnt[i] = static_cast<unsigned char>(n);
    }
    __syncthreads();

    // ---- the (pattern, anchor) pairs, pattern-major; the cheap atom-0 test comes first inside sub_search ----
    const int pairs = n_patterns * N;                               // <= 1024 * 256
    for (int item = tid; item < pairs; item += nt) {
        const int p = item / N, a = item - p * N;
        if (!(prop[a] & SUB_IN_SCOPE)) continue;
        const unsigned* pat = patterns + static_cast<size_t>(p) * SUB_WORDS;
        int steps;
        const int found = sub_search(pat, prop, sets, ncnt, nbr, a, image + tid, cursor + tid, MS_MAX, &steps);
        if (found == SUB_MATCH) {
            atomicAdd(&hit[p], 1);
            if ((pat[0] >> 16) & DG_SUB_TYPING) atomicMin(&atype[a], p);
        } else if (found == SUB_OVER) {
            atomicAdd(&over, 1u);
        }
    }
    __syncthreads();

    // ---- the types are final: the sums, the outputs ----
    unsigned heavy = 0u, typed = 0u, sum0 = 0u, sum1 = 0u, n_hit = 0u;
    for (int i = tid; i < N; i += nt) {
        const unsigned p = prop[i];
        const int t = atype[i];
        const bool in = p & SUB_IN_SCOPE, has = in && t != MS_NONE;
        atom_type[b * N + i] = has ? t : -1;
        heavy += in;
        typed += has;
        if (has) {
            const unsigned* pat = patterns + static_cast<size_t>(t) * SUB_WORDS;
            const unsigned h = p & 15u;
            sum0 += pat[1] + h * pat[2];
            sum1 += pat[3] + h * pat[4];
        }
    }
    for (int p = tid; p < n_patterns; p += nt) {
        const int v = hit[p];
        hits[b * n_patterns + p] = v;
        n_hit += v > 0;
    }
    heavy = wave_usum(heavy);
    typed = wave_usum(typed);
    sum0 = wave_usum(sum0);
    sum1 = wave_usum(sum1);
    n_hit = wave_usum(n_hit);
    if ((tid & 63) == 0) {
        unsigned* mine = part[tid >> 6];
        mine[T_HEAVY] = heavy;
        mine[T_TYPED] = typed;
        mine[T_SUM0] = sum0;
        mine[T_SUM1] = sum1;
        mine[T_HIT] = n_hit;
    }
    __syncthreads();
    if (tid < DG_SUB_MOL_FIELDS) {
        unsigned tot[T_COUNT] = {0u, 0u, 0u, 0u, 0u};
        for (int w = 0; w < nt >> 6; ++w)
            for (int k = 0; k < T_COUNT; ++k) tot[k] += part[w][k];
        unsigned v = 0u;
        if (tid == 0) v = static_cast<unsigned>(status);
        else if (tid == 1) v = tot[T_HEAVY];
        else if (tid == 2) v = tot[T_TYPED];
        else if (tid == 3) v = tot[T_HEAVY] - tot[T_TYPED];
        else if (tid == 4) v = tot[T_SUM0];
        else if (tid == 5) v = tot[T_SUM1];
        else if (tid == 6) v = tot[T_HIT];
        else v = over;
        mol[b * DG_SUB_MOL_FIELDS + tid] = static_cast<int>(v);
    }
}

}  // namespace
}  // namespace dg

using namespace dg;

extern "C" int dg_mol_substructure(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds, const int* desc,
                                   const unsigned* atom_key, const unsigned char* bond_class, const unsigned* bond_table,
                                   int n_bond_labels, const unsigned* atom_sets, int n_atom_labels, const unsigned* patterns,
                                   int n_patterns, int B, int N, int cap, int* mol, int* hits, int* atom_type,
                                   dg_stream_t stream_) {
    if (B < 0 || N < 1 || N > 256 || cap < 0 || n_atom_labels < 1 || n_atom_labels > 255 || n_bond_labels < 1 ||
        n_bond_labels > 256 || n_patterns < 0 || n_patterns > DG_SUB_MAX_PATTERNS)
        return fail(DG_E_SHAPE, "dg_mol_substructure: need B >= 0, 1 <= N <= 256, cap >= 0, 1 <= n_atom_labels <= 255, "
                    "1 <= n_bond_labels <= 256, 0 <= n_patterns <= %d (B=%d N=%d cap=%d n_atom_labels=%d n_bond_labels=%d "
                    "n_patterns=%d)", DG_SUB_MAX_PATTERNS, B, N, cap, n_atom_labels, n_bond_labels, n_patterns);
    if (!atoms || !n_bonds || !desc || !atom_key || !bond_table || !atom_sets || !mol || !atom_type)
        return fail(DG_E_ARG, "dg_mol_substructure: null pointer");
    if (cap > 0 && (!bonds || !bond_class)) return fail(DG_E_ARG, "dg_mol_substructure: null pointer (bonds / bond_class with cap > 0)");
    if (n_patterns > 0 && (!patterns || !hits))
        return fail(DG_E_ARG, "dg_mol_substructure: null pointer (patterns / hits with n_patterns > 0)");
    if (misaligned(bonds, 4) || misaligned(n_bonds, 4) || misaligned(desc, 4) || misaligned(atom_key, 4) ||
        misaligned(bond_table, 4) || misaligned(atom_sets, 4) || misaligned(patterns, 4) || misaligned(mol, 4) ||
        misaligned(hits, 4) || misaligned(atom_type, 4))
        return fail(DG_E_ARG, "dg_mol_substructure: bond rows, tables, int arrays, desc, atom_key and the outputs must be 4-byte aligned");
    if (B == 0) return 0;
    const int pairs = N * max(n_patterns, 1);                       // <= 2^18; whole waves, no more than the pairs can use
    const int threads = min(256, max(64, (pairs + 63) & ~63));
    hipLaunchKernelGGL(mol_sub_kernel, dim3(static_cast<unsigned>(B)), dim3(threads), 0, static_cast<hipStream_t>(stream_), atoms,
                       reinterpret_cast<const unsigned*>(bonds), n_bonds, desc, atom_key, bond_class, bond_table, n_bond_labels,
                       atom_sets, n_atom_labels, patterns, n_patterns, N, cap, mol, hits, atom_type);
    return check_launch("dg_mol_substructure");
}
