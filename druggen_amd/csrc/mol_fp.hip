// Circular fingerprints of a decoded batch (dg_mol_fingerprint of include/druggen_hip_fp.h): what
// druggen_amd/metrics.py starts from, made on the device.  Integers only, no atomics but LDS integer ones (exact in any
// order), every loop carries its trip limit, nothing waits on another workgroup.
//
//   mol_fp_kernel   one workgroup per molecule, one thread per atom (64..256 threads).  LDS holds the adjacency bit rows, the
//                   ids of every layer, the growing balls and, per layer and atom, the atom set K that stands for the
//                   environment (two environments are equal exactly when their K are).  The bond list stays in
//                   global memory and is walked once per phase -- scope, degrees, ring flags, every layer's neighbour sums --
//                   so no bond count is refused.  A hash of K selects candidates, the words of K decide.
#include "mol_key.h"
#include "mol_ring.h"
#include "../../include/druggen_hip_fp.h"

namespace dg {
namespace {

constexpr int MFP_MAX = 256;                                     // atoms, labels, threads
typedef unsigned long long u64;

// ids of R + 1 layers, the neighbour sums, adjacency + two balls + R layers of K, R layers of hashes
__host__ __device__ constexpr int lds_bytes(int N, int R) {
    return (R + 2) * N * 8 + (3 + R) * N * row_stride(N) * 4 + R * N * 4;
}

__global__ __launch_bounds__(MFP_MAX) void mol_fp_kernel(
    const unsigned char* __restrict__ atoms, const unsigned* __restrict__ bonds, const int* __restrict__ n_bonds,
    const unsigned char* __restrict__ component, const int* __restrict__ largest, const int* __restrict__ flags,
    const unsigned* __restrict__ atom_words, int n_atom_labels, const unsigned* __restrict__ bond_table, int n_bond_labels, int N,
    int cap, int scope, int R, int nbits, int* __restrict__ words, int* __restrict__ counts, int* __restrict__ n_features) {
    extern __shared__ __align__(16) unsigned char dyn[];
    const int W = (N + 31) >> 5, S = row_stride(N);
    u64* ids = reinterpret_cast<u64*>(dyn);                         // ids[r * N + a], r = 0..R
    u64* acc = ids + (R + 1) * N;                                   // the neighbour sum of the layer under way
    unsigned* adj = reinterpret_cast<unsigned*>(acc + N);           // adj[v * S + w]: bits 32 w .. 32 w + 31 of atom v's row
    unsigned* ball_a = adj + N * S;                                 // the ball of layer r (odd r here, even r in ball_b)
    unsigned* ball_b = ball_a + N * S;
    unsigned* kset = ball_b + N * S;                                // kset[((r - 1) * N + a) * S + w]
    unsigned* khash = kset + R * N * S;                             // khash[(r - 1) * N + a]
    __shared__ u64 mbw[MFP_MAX];                                    // M(word of the bond label)
    __shared__ unsigned aw[MFP_MAX], ord2[MFP_MAX], deg[MFP_MAX], val2[MFP_MAX];
    __shared__ unsigned short parent[MFP_MAX], depth[MFP_MAX];      // the breadth-first forest
    __shared__ unsigned char lab_a[MFP_MAX], member[MFP_MAX], ring[MFP_MAX], cov[MFP_MAX];      // cov: the bond to the parent is on a cycle
    __shared__ unsigned char cand[(DG_FP_MAX_RADIUS + 1) * MFP_MAX];      // cand[r * 256 + a]: id_r[a] is a feature
    __shared__ unsigned front[8], vis[8], bonded[8], out_w[128];
    __shared__ int totals[2];                                       // features, set bits

    const int tid = threadIdx.x, nt = blockDim.x;                   // nt >= N
    const int64_t b = blockIdx.x;
    const int NW = nbits >> 5;
    int* w_row = words + b * NW;
    const int nb = n_bonds[b];
    if (nb > cap || (flags && flags[b] < 0)) {                      // no graph (uniform over the workgroup)
        for (int i = tid; i < NW; i += nt) w_row[i] = 0;
        if (tid == 0) {
            counts[b] = 0;
            n_features[b] = DG_FP_NO_GRAPH;
        }
        return;
    }
    const int kept = max(nb, 0);
    const unsigned* list = bonds + b * cap;

    for (int w = tid; w < N * S; w += nt) adj[w] = 0u;
    for (int i = tid; i < MFP_MAX; i += nt) {
        deg[i] = val2[i] = 0u;
        parent[i] = RING_NONE;
        depth[i] = 0;
        member[i] = ring[i] = cov[i] = 0;
        lab_a[i] = i < N ? atoms[b * N + i] : 0;
        aw[i] = i < n_atom_labels ? atom_words[i] : 0xFFFFFFFFu;
        mbw[i] = mix64(i < n_bond_labels ? bond_table[2 * i] : 0xFFFFFFFFu);
        ord2[i] = i < n_bond_labels ? bond_table[2 * i + 1] : 0u;
    }
    for (int i = tid; i < (DG_FP_MAX_RADIUS + 1) * MFP_MAX; i += nt) cand[i] = 0;
    for (int i = tid; i < 128; i += nt) out_w[i] = 0u;
    if (tid < 8) front[tid] = vis[tid] = bonded[tid] = 0u;
    if (tid < 2) totals[tid] = 0;
    __syncthreads();

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

    // ---- the bonds inside it: degrees, twice the valence, bit rows ----
    for (int k = tid; k < kept; k += nt) {
        const unsigned row = list[k];
        const int i = row & 255u, j = (row >> 8) & 255u;
        if (i >= N || j >= N || i == j || !member[i] || !member[j]) continue;
        const unsigned o = ord2[(row >> 16) & 255u];
        atomicAdd(&deg[i], 1u);
        atomicAdd(&deg[j], 1u);
        atomicAdd(&val2[i], o);
        atomicAdd(&val2[j], o);
        atomicOr(&adj[i * S + (j >> 5)], 1u << (j & 31));
        atomicOr(&adj[j * S + (i >> 5)], 1u << (i & 31));
    }
    __syncthreads();
    if (tid < N && deg[tid]) atomicOr(&bonded[tid >> 5], 1u << (tid & 31));

    // ---- ring flags (mol_ring.h): a breadth-first forest, then the tree paths that the bonds outside it close ----
    ring_forest(N, adj, deg, bonded, front, vis, parent, depth);
    ring_cover(N, list, kept, member, parent, depth, cov, ring);
    __syncthreads();
    if (tid < N && cov[tid]) {
        ring[tid] = 1;
        ring[parent[tid]] = 1;
    }
    __syncthreads();

    // ---- layer 0 ----
    if (tid < N && member[tid]) {
        u64 t = mix64(aw[lab_a[tid]]);
        t = mix64(t + deg[tid]);
        t = mix64(t + val2[tid]);
        ids[tid] = mix64(t + ring[tid]);
        cand[tid] = 1;
        for (int w = 0; w < W; ++w) ball_a[tid * S + w] = 0u;
        ball_a[tid * S + (tid >> 5)] = 1u << (tid & 31);
    }

    // ---- layers 1..R ----
    for (int r = 1; r <= R; ++r) {
        const u64* prev = ids + (r - 1) * N;
        u64* now = ids + r * N;
        if (tid < N) acc[tid] = 0ull;
        __syncthreads();                                            // prev is complete
        for (int k = tid; k < kept; k += nt) {
            const unsigned row = list[k];
            const int i = row & 255u, j = (row >> 8) & 255u;
            if (i >= N || j >= N || i == j || !member[i] || !member[j]) continue;
            const u64 m = mbw[(row >> 16) & 255u];
            atomicAdd(&acc[i], mix64(prev[j] + m));
            atomicAdd(&acc[j], mix64(prev[i] + m));
        }
        __syncthreads();
        const unsigned* cur = (r & 1) ? ball_a : ball_b;            // atoms within distance r - 1
        unsigned* nxt = (r & 1) ? ball_b : ball_a;                  // ... within distance r
        unsigned* my_k = kset + ((r - 1) * N + tid) * S;
        const bool live = tid < N && member[tid] && deg[tid];
        if (tid < N && member[tid]) now[tid] = mix64(mix64(prev[tid] + static_cast<u64>(r)) + acc[tid]);
        if (live) {
            const int a = tid;
            for (int w = 0; w < W; ++w) nxt[a * S + w] = cur[a * S + w];
            for (int w = 0; w < W; ++w) {
                unsigned word = cur[a * S + w];
                while (word) {
                    const int x = 32 * w + __ffs(word) - 1;
                    word &= word - 1u;
                    for (int w2 = 0; w2 < W; ++w2) nxt[a * S + w2] |= adj[x * S + w2];
                }
            }
            // K = the ball and every atom all of whose neighbours are in it (such an atom is a neighbour of the ball)
            u64 h = 0ull;
            for (int w = 0; w < W; ++w) {
                unsigned kw = cur[a * S + w];
                unsigned rim = nxt[a * S + w] & ~kw;
                while (rim) {
                    const int bit = __ffs(rim) - 1;
                    rim &= rim - 1u;
                    const int x = 32 * w + bit;
                    unsigned outside = 0u;
                    for (int w2 = 0; w2 < W; ++w2) outside |= adj[x * S + w2] & ~cur[a * S + w2];
                    if (!outside) kw |= 1u << bit;
                }
                my_k[w] = kw;
                h += mix(static_cast<unsigned>(w), kw);
            }
            khash[(r - 1) * N + a] = static_cast<unsigned>(h ^ (h >> 32));
        }
        __syncthreads();                                            // ids, K and hashes of layer r are complete
        if (live) {
            const int a = tid;
            const unsigned mine = khash[(r - 1) * N + a];
            const u64 my_id = now[a];
            bool keep = true;
            for (int r2 = 1; r2 <= r && keep; ++r2) {
                const unsigned* hashes = khash + (r2 - 1) * N;
                for (int x = 0; x < N; ++x) {
                    if (hashes[x] != mine || !member[x] || !deg[x] || (r2 == r && x == a)) continue;
                    const unsigned* other = kset + ((r2 - 1) * N + x) * S;
                    bool same = true;
                    for (int w = 0; w < W; ++w) same &= other[w] == my_k[w];
                    if (!same) continue;
                    // seen at a lower layer; or at this one by an atom with a smaller id (ties: the smaller index)
                    if (r2 < r || now[x] < my_id || (now[x] == my_id && x < a)) {
                        keep = false;
                        break;
                    }
                }
            }
            cand[r * MFP_MAX + a] = keep;
        }
    }
    __syncthreads();

    // ---- F as a set of values: a candidate counts unless an earlier one (layer, then atom) has its value ----
    if (tid < N && member[tid]) {
        const int a = tid;
        for (int r = 0; r <= R; ++r) {
            if (!cand[r * MFP_MAX + a]) continue;
            const u64 v = ids[r * N + a];
            bool dup = false;
            for (int r2 = 0; r2 <= r && !dup; ++r2) {
                const int end = r2 < r ? N : a;
                for (int x = 0; x < end; ++x) {
                    if (cand[r2 * MFP_MAX + x] && ids[r2 * N + x] == v) {
                        dup = true;
                        break;
                    }
                }
            }
            if (dup) continue;
            atomicAdd(&totals[0], 1);
            const unsigned bit = static_cast<unsigned>(v % static_cast<u64>(nbits));
            atomicOr(&out_w[bit >> 5], 1u << (bit & 31));
        }
    }
    __syncthreads();
    for (int i = tid; i < NW; i += nt) {
        const unsigned w = out_w[i];
        w_row[i] = static_cast<int>(w);
        if (w) atomicAdd(&totals[1], __popc(w));
    }
    __syncthreads();
    if (tid == 0) {
        counts[b] = totals[1];
        n_features[b] = totals[0];
    }
}

}  // namespace
}  // namespace dg

using namespace dg;

extern "C" int dg_mol_fingerprint(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds,
                                  const unsigned char* component, const int* largest, const int* flags,
                                  const unsigned* atom_words, int n_atom_labels, const unsigned* bond_table, int n_bond_labels,
                                  int B, int N, int cap, int scope, int radius, int nbits, int* words, int* counts,
                                  int* n_features, dg_stream_t stream_) {
    if (B < 0 || N < 1 || N > 256 || cap < 0 || radius < 0 || radius > DG_FP_MAX_RADIUS || nbits < 32 || nbits > 4096 ||
        (nbits & 31) || n_atom_labels < 1 || n_atom_labels > 255 || n_bond_labels < 1 || n_bond_labels > 256)
        return fail(DG_E_SHAPE, "dg_mol_fingerprint: need B >= 0, 1 <= N <= 256, cap >= 0, 0 <= radius <= 4, nbits a multiple of "
                    "32 in 32..4096, 1 <= n_atom_labels <= 255, 1 <= n_bond_labels <= 256 (B=%d N=%d cap=%d radius=%d nbits=%d "
                    "n_atom_labels=%d n_bond_labels=%d)", B, N, cap, radius, nbits, n_atom_labels, n_bond_labels);
    if (scope != DG_CANON_WHOLE && scope != DG_CANON_LARGEST)
        return fail(DG_E_ARG, "dg_mol_fingerprint: scope must be 0 (whole) or 1 (largest), got %d", scope);
    if (!atoms || !n_bonds || !atom_words || !bond_table || !words || !counts || !n_features)
        return fail(DG_E_ARG, "dg_mol_fingerprint: null pointer");
    if (scope == DG_CANON_LARGEST && (!component || !largest))
        return fail(DG_E_ARG, "dg_mol_fingerprint: null pointer (component / largest with scope 1)");
    if (cap > 0 && !bonds) return fail(DG_E_ARG, "dg_mol_fingerprint: null pointer (bonds with cap > 0)");
    if (misaligned(bonds, 4) || misaligned(n_bonds, 4) || misaligned(largest, 4) || misaligned(flags, 4) ||
        misaligned(atom_words, 4) || misaligned(bond_table, 4) || misaligned(words, 4) || misaligned(counts, 4) ||
        misaligned(n_features, 4))
        return fail(DG_E_ARG, "dg_mol_fingerprint: bond rows, tables and int arrays must be 4-byte aligned");
    if (B == 0) return 0;
    DG_OPT_IN_LDS(&mol_fp_kernel, lds_bytes(MFP_MAX, DG_FP_MAX_RADIUS));
    const int threads = max(64, (N + 63) & ~63);                    // one thread per atom, whole waves
    hipLaunchKernelGGL(mol_fp_kernel, dim3(static_cast<unsigned>(B)), dim3(threads), static_cast<size_t>(lds_bytes(N, radius)),
                       static_cast<hipStream_t>(stream_), atoms, reinterpret_cast<const unsigned*>(bonds), n_bonds, component,
                       largest, flags, atom_words, n_atom_labels, bond_table, n_bond_labels, N, cap, scope, radius, nbits, words,
                       counts, n_features);
    return check_launch("dg_mol_fingerprint");
}
