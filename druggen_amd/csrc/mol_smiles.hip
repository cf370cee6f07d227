// SMILES strings of a decoded batch (dg_mol_smiles of include/druggen_hip_text.h): the reference's end product
// (mol_sample / save_smiles_matrices of src/util/utils.py, inference.py) written on the device, in the dialect
// druggen_amd/smiles.py reads.  Integers only, no atomics but the LDS ors that build the bit rows, every loop carries its trip
// limit, nothing waits on another workgroup.
//
//   mol_smiles_kernel   one wave per molecule.  The 64 lanes build the graph in LDS the way mol_canon.hip keeps it -- bit rows
//                       and the packed lower triangle of labels, here over atom positions (the traversal order is defined on
//                       them) -- lane 0 walks it twice: a depth-first search (preorder, parent, last child), then the string in
//                       preorder, staged in LDS; the 64 lanes write the string and the order out, four bytes per lane where the
//                       rows allow it.
#include "common.h"
#include "../../include/druggen_hip_text.h"

namespace dg {
namespace {

constexpr int MSM_THREADS = 64;
constexpr int MSM_NONE = 0xFFFF;                             // no parent / no child
constexpr int MSM_RINGS = 99;                                // ring numbers 1..99

__device__ __forceinline__ int tri(int i) { return (i * (i - 1)) >> 1; }      // offset of row i in the packed lower triangle

__host__ __device__ constexpr int round4(int x) { return (x + 3) & ~3; }

// the open ring numbers: bit n - 1 of a 128-bit set
struct RingSet {
    unsigned long long lo, hi;
    __device__ void set(int i) { if (i < 64) lo |= 1ull << i; else hi |= 1ull << (i - 64); }
    __device__ int first_free() const {                     // smallest i in 0..98 that is not in the set, -1: none
        if (~lo) return __ffsll(static_cast<long long>(~lo)) - 1;
        const unsigned long long free = ~hi & ((1ull << (MSM_RINGS - 64)) - 1ull);
        return free ? 64 + __ffsll(static_cast<long long>(free)) - 1 : -1;
    }
};

__global__ __launch_bounds__(MSM_THREADS) void mol_smiles_kernel(
    const unsigned char* __restrict__ atoms, const unsigned* __restrict__ bonds, const int* __restrict__ n_bonds,
    const unsigned char* __restrict__ component, const int* __restrict__ largest, const int* __restrict__ flags,
    const unsigned char* __restrict__ atom_table, int n_atom_labels, const unsigned char* __restrict__ bond_table,
    int n_bond_labels, int N, int cap, int scope, int str_cap, int wide, int* __restrict__ length, int* __restrict__ n_written,
    unsigned char* __restrict__ order, unsigned char* __restrict__ text) {
    extern __shared__ __align__(16) unsigned char dyn[];
    const int W = (N + 31) >> 5;                                    // 32-bit words of a bit row
    const int cap4 = round4(str_cap);
    unsigned* adj = reinterpret_cast<unsigned*>(dyn);               // adj[v * W + w]: bits 32 w .. 32 w + 31 of atom v's row
    unsigned char* txt = dyn + N * W * 4;                           // the string, zero past its end
    unsigned char* lab = txt + cap4;                                // bond labels between atoms hi > lo: lab[tri(hi) + lo]
    __shared__ unsigned short parent[256], last[256], cur[256];     // tree parent, last tree child, next neighbour to try
    __shared__ unsigned short ring_a[MSM_RINGS + 1], ring_d[MSM_RINGS + 1];      // the two ends of the ring bond that holds a number
    __shared__ unsigned char ord[256], pre[256], lab_a[256], member[256], arom[256], low[256], seen[256];
    __shared__ unsigned char atab[256 * 4], btab[256 * 2];
    __shared__ unsigned ring_at[8];                                 // ring bonds of one atom as bits over preorder positions
    __shared__ int result[2];                                       // length / status, atoms of the scope

    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    unsigned char* ord_row = order + b * N;
    unsigned char* txt_row = text + b * str_cap;
    const int nb = n_bonds[b];
    if (nb > cap || (flags && flags[b] < 0)) {                      // no graph (uniform over the wave)
        for (int i = tid; i < N; i += MSM_THREADS) ord_row[i] = 0xFF;
        if (wide) {
            for (int i = tid; i < (str_cap >> 2); i += MSM_THREADS) reinterpret_cast<unsigned*>(txt_row)[i] = 0u;
        } else {
            for (int i = tid; i < str_cap; i += MSM_THREADS) txt_row[i] = 0;
        }
        if (tid == 0) {
            length[b] = DG_SMILES_NO_GRAPH;
            n_written[b] = 0;
        }
        return;
    }
    const int kept = max(nb, 0);
    const unsigned* list = bonds + b * cap;

    for (int w = tid; w < N * W; w += MSM_THREADS) adj[w] = 0u;
    for (int w = tid; w < (cap4 >> 2); w += MSM_THREADS) reinterpret_cast<unsigned*>(txt)[w] = 0u;
    for (int i = tid; i < 256; i += MSM_THREADS) {
        parent[i] = last[i] = MSM_NONE;
        cur[i] = 0;
        member[i] = arom[i] = seen[i] = 0;
        lab_a[i] = i < N ? atoms[b * N + i] : 0;
        const bool known = i < n_atom_labels && atom_table[4 * i] != 0;
        atab[4 * i] = known ? atom_table[4 * i] : '?';
        atab[4 * i + 1] = known ? atom_table[4 * i + 1] : 0;
        atab[4 * i + 2] = known ? atom_table[4 * i + 2] : 0;
        const bool bond_known = i < n_bond_labels && bond_table[2 * i] != 0;
        btab[2 * i] = bond_known ? bond_table[2 * i] : '?';
        btab[2 * i + 1] = bond_known ? bond_table[2 * i + 1] : 0;
    }
    __syncthreads();

    // ---- the scope ----
    if (scope == DG_CANON_WHOLE) {
        for (int k = tid; k < kept; k += MSM_THREADS) {
            const unsigned row = list[k];
            const int i = row & 255u, j = (row >> 8) & 255u;
            if (i < N && j < N && i != j) member[i] = member[j] = 1;
        }
        __syncthreads();
        for (int i = tid; i < N; i += MSM_THREADS) member[i] = member[i] || lab_a[i] != 0;
    } else if (scope == DG_CANON_LARGEST) {
        const int root = largest[b];
        for (int i = tid; i < N; i += MSM_THREADS) member[i] = component[b * N + i] == root;
    } else {
        for (int i = tid; i < N; i += MSM_THREADS) member[i] = lab_a[i] != 0xFF;
    }
    __syncthreads();

    // ---- the bonds inside it ----
    for (int k = tid; k < kept; k += MSM_THREADS) {
        const unsigned row = list[k];
        const int i = row & 255u, j = (row >> 8) & 255u;
        if (i >= N || j >= N || i == j || !member[i] || !member[j]) continue;
        const int hi = max(i, j), lo = min(i, j);
        const unsigned l = (row >> 16) & 255u;
        lab[tri(hi) + lo] = static_cast<unsigned char>(l);
        atomicOr(&adj[hi * W + (lo >> 5)], 1u << (lo & 31));
        atomicOr(&adj[lo * W + (hi >> 5)], 1u << (hi & 31));
        if (btab[2 * l + 1]) arom[i] = arom[j] = 1;
    }
    __syncthreads();
    for (int i = tid; i < N; i += MSM_THREADS) low[i] = arom[i] && (atab[4 * lab_a[i] + 2] & 2);
    __syncthreads();

    if (tid == 0) {
        // ---- the traversal: a step takes one neighbour bit (2 bonds in all) or returns to the parent (once per atom) ----
        int count = 0, steps = 0;
        const int limit = 2 * (N + min(kept, tri(N)));
        for (int root = 0; root < N; ++root) {
            if (!member[root] || seen[root]) continue;
            seen[root] = 1;
            pre[root] = static_cast<unsigned char>(count);
            ord[count++] = static_cast<unsigned char>(root);
            int v = root;
            while (steps++ < limit) {
                const int from = cur[v];
                int u = -1;
                for (int w = from >> 5; w < W; ++w) {
                    unsigned word = adj[v * W + w];
                    if (w == (from >> 5)) word &= ~0u << (from & 31);
                    if (word) {
                        u = 32 * w + __ffs(word) - 1;
                        break;
                    }
                }
                if (u < 0) {
                    cur[v] = static_cast<unsigned short>(32 * W);
                    const int p = parent[v];
                    if (p == MSM_NONE) break;
                    v = p;
                    continue;
                }
                cur[v] = static_cast<unsigned short>(u + 1);
                if (!seen[u]) {
                    seen[u] = 1;
                    parent[u] = static_cast<unsigned short>(v);
                    last[v] = static_cast<unsigned short>(u);
                    pre[u] = static_cast<unsigned char>(count);
                    ord[count++] = static_cast<unsigned char>(u);
                    v = u;
                }
            }
        }

        // ---- the string, atom by atom in preorder; past str_cap the position still counts ----
        int at = 0;
        bool rings_out = false;
        RingSet open{0ull, 0ull}, closed{0ull, 0ull};               // numbers in use; those closed at the current atom
        auto put = [&](unsigned ch) {
            if (at < str_cap) txt[at] = static_cast<unsigned char>(ch);
            ++at;
        };
        auto put_bond = [&](int x, int y) {
            const unsigned l = lab[tri(max(x, y)) + min(x, y)];
            const unsigned sym = btab[2 * l];
            if (low[x] && low[y] ? !btab[2 * l + 1] : sym != '-') put(sym);
        };
        auto put_number = [&](int n) {
            if (n >= 10) {
                put('%');
                put('0' + n / 10);
            }
            put('0' + n % 10);
        };
        for (int k = 0; k < count && !rings_out; ++k) {
            const int v = ord[k], p = parent[v];
            if (p == MSM_NONE) {
                if (k) put('.');
            } else {
                if (last[p] != v) put('(');
                put_bond(p, v);
            }
            {
                const unsigned l = lab_a[v], fl = atab[4 * l + 2], second = atab[4 * l + 1];
                if (fl & 1u) put('[');
                put(low[v] ? atab[4 * l] | 0x20u : atab[4 * l]);
                if (second) put(second);
                if (fl & 1u) put(']');
            }
            open.lo &= ~closed.lo;
            open.hi &= ~closed.hi;
            closed = RingSet{0ull, 0ull};
            // the ring bonds of v, sorted by the other end's preorder position: bits over those positions
            for (int w = 0; w < 8; ++w) ring_at[w] = 0u;
            for (int w = 0; w < W; ++w) {
                unsigned word = adj[v * W + w];
                while (word) {
                    const int u = 32 * w + __ffs(word) - 1;
                    word &= word - 1u;
                    if (u != p && parent[u] != v) ring_at[pre[u] >> 5] |= 1u << (pre[u] & 31);
                }
            }
            for (int w = 0; w < 8 && !rings_out; ++w) {
                unsigned word = ring_at[w];
                while (word) {
                    const int q = 32 * w + __ffs(word) - 1;
                    word &= word - 1u;
                    const int u = ord[q];
                    if (q < k) {                                    // closes the ring u opened for v
                        int n = -1;
                        for (int half = 0; half < 2 && n < 0; ++half) {
                            unsigned long long in_use = half ? open.hi : open.lo;
                            while (in_use) {                        // at most 99 numbers
                                const int i = 64 * half + __ffsll(static_cast<long long>(in_use)) - 1;
                                in_use &= in_use - 1ull;
                                if (ring_a[i] == u && ring_d[i] == v) {
                                    n = i;
                                    break;
                                }
                            }
                        }
                        if (n < 0) continue;                        // (every ring bond to an ancestor was opened there)
                        put_bond(u, v);
                        put_number(n + 1);
                        closed.set(n);
                    } else {
                        const int n = open.first_free();
                        if (n < 0) {
                            rings_out = true;
                            break;
                        }
                        open.set(n);
                        ring_a[n] = static_cast<unsigned short>(v);
                        ring_d[n] = static_cast<unsigned short>(u);
                        put_number(n + 1);
                    }
                }
            }
            if (last[v] == MSM_NONE) {                              // a leaf ends the branch it is the last atom of
                int u = v;
                for (int t = 0; t < N; ++t) {
                    const int pp = parent[u];
                    if (pp == MSM_NONE) break;
                    if (last[pp] != u) {
                        put(')');
                        break;
                    }
                    u = pp;
                }
            }
        }
        result[0] = rings_out ? DG_SMILES_RINGS : at > str_cap ? DG_SMILES_LONG : at;
        result[1] = count;
    }
    __syncthreads();

    const int len = result[0], count = result[1];
    for (int i = tid; i < N; i += MSM_THREADS) ord_row[i] = i < count ? ord[i] : 0xFF;
    if (wide) {                                                     // the string is zero past len in LDS
        for (int i = tid; i < (str_cap >> 2); i += MSM_THREADS)
            reinterpret_cast<unsigned*>(txt_row)[i] = len >= 0 ? reinterpret_cast<const unsigned*>(txt)[i] : 0u;
    } else {
        for (int i = tid; i < str_cap; i += MSM_THREADS) txt_row[i] = len >= 0 ? txt[i] : 0;
    }
    if (tid == 0) {
        length[b] = len;
        n_written[b] = count;
    }
}

}  // namespace
}  // namespace dg

using namespace dg;

extern "C" int dg_mol_smiles(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds,
                             const unsigned char* component, const int* largest, const int* flags,
                             const unsigned char* atom_table, int n_atom_labels, const unsigned char* bond_table,
                             int n_bond_labels, int B, int N, int cap, int scope, int str_cap, int* length, int* n_written,
                             unsigned char* order, unsigned char* text, dg_stream_t stream_) {
    if (B < 0 || N < 1 || N > 256 || cap < 0 || str_cap < 1 || n_atom_labels < 1 || n_atom_labels > 255 || n_bond_labels < 1 ||
        n_bond_labels > 256)
        return fail(DG_E_SHAPE, "dg_mol_smiles: need B >= 0, 1 <= N <= 256, cap >= 0, str_cap >= 1, 1 <= n_atom_labels <= 255, "
                    "1 <= n_bond_labels <= 256 (B=%d N=%d cap=%d str_cap=%d n_atom_labels=%d n_bond_labels=%d)", B, N, cap, str_cap,
                    n_atom_labels, n_bond_labels);
    const int graph_bytes = N * ((N + 31) >> 5) * 4 + round4(N * (N - 1) / 2);
    if (str_cap > DG_SMILES_MAX_LDS - graph_bytes)                  // (both multiples of 4: the rounded str_cap fits too)
        return fail(DG_E_SHAPE, "dg_mol_smiles: str_cap = %d does not fit LDS next to the graph of N = %d atoms (%d of %d bytes)",
                    str_cap, N, graph_bytes, DG_SMILES_MAX_LDS);
    if (scope != DG_CANON_WHOLE && scope != DG_CANON_LARGEST && scope != DG_SMILES_FORMS)
        return fail(DG_E_ARG, "dg_mol_smiles: scope must be 0 (whole), 1 (largest) or 2 (forms), got %d", scope);
    if (!atoms || !n_bonds || !atom_table || !bond_table || !length || !n_written || !order || !text)
        return fail(DG_E_ARG, "dg_mol_smiles: null pointer");
    if (scope == DG_CANON_LARGEST && (!component || !largest))
        return fail(DG_E_ARG, "dg_mol_smiles: null pointer (component / largest with scope 1)");
    if (cap > 0 && !bonds) return fail(DG_E_ARG, "dg_mol_smiles: null pointer (bonds with cap > 0)");
    if (misaligned(bonds, 4) || misaligned(n_bonds, 4) || misaligned(largest, 4) || misaligned(flags, 4) ||
        misaligned(length, 4) || misaligned(n_written, 4))
        return fail(DG_E_ARG, "dg_mol_smiles: bond rows and int arrays must be 4-byte aligned");
    if (B == 0) return 0;
    const size_t lds = static_cast<size_t>(graph_bytes + round4(str_cap));
    const int wide = (str_cap & 3) == 0 && !misaligned(text, 4);    // every row of text starts on a 4-byte boundary
    hipLaunchKernelGGL(mol_smiles_kernel, dim3(static_cast<unsigned>(B)), dim3(MSM_THREADS), lds,
                       static_cast<hipStream_t>(stream_), atoms, reinterpret_cast<const unsigned*>(bonds), n_bonds, component,
                       largest, flags, atom_table, n_atom_labels, bond_table, n_bond_labels, N, cap, scope, str_cap, wide, length,
                       n_written, order, text);
    return check_launch("dg_mol_smiles");
}
