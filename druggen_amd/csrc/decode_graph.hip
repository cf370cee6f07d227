// Graph decode of a generated batch -- what the reference does on the host, one molecule at a time, between the
// generator and RDKit (inference.py:197-206: torch.max(.., -1)[1], `.cpu().numpy()` per molecule; dataset.py:218-223:
// np.nonzero over the dense bond matrix, keep start > end):
//   atoms[i] = argmax_m node[i,:],  l[i,j] = argmax_e edge[i,j,:]  (first maximum, NaN maximal: the rule of argmax_kernel)
//   bond list (i, j, l[i,j]) over i > j with l != 0, ascending i then j;  connected components of that graph (label =
//   smallest atom index), their count, the largest one;  twice the valence of every atom.
// Every output is an integer function of the labels: exact, independent of wave timing.
//
// One workgroup of 256 lanes per molecule.  The molecule's [N, N, E] logits are its only real HBM stream; rows of E floats
// are not 16-byte aligned (E = 5), so the block is streamed as ALIGNED float4s through a 16 KiB LDS tile (registers hold the
// next tile while this one is reduced) and every lane picks whole pairs out of LDS.  Lower-triangle labels stay in LDS as
// bytes (packed triangle, <= 32 640 B), the adjacency as bit rows (8 KiB, word-major: lane i reads word w of row i without
// bank conflicts).
#include "common.h"

namespace dg {
namespace {

constexpr int DGR_THREADS = 256;
constexpr int DGR_STAGE_F4 = 1024;                           // float4 slots of the staging tile: four per lane
constexpr int DGR_PAIR_FLOATS = 4 * DGR_STAGE_F4 - 8;        // floats of whole pairs per tile (<= 3 + 3 floats of alignment slack)
constexpr int DGR_WORDS = 8;                                 // 32-bit words of a bit row (N <= 256)

__device__ __forceinline__ int tri(int i) { return (i * (i - 1)) >> 1; }      // offset of row i in the packed lower triangle

// index of the first maximum of x[0..n), NaN counts as maximal (torch.max / argmax_kernel of aux_kernels.hip)
__device__ __forceinline__ int first_max(const float* x, int n) {
    float best = x[0];
    int arg = 0;
    for (int c = 1; c < n; ++c) {
        const float v = x[c];
        if (v > best || (v != v && best == best)) {
            best = v;
            arg = c;
        }
    }
    return arg;
}

// The same over a row in GLOBAL memory (the node logits: one short row per lane, read once): the loads of a group are issued
// together, so a row of 13 costs three memory latencies, not thirteen.
__device__ __forceinline__ int first_max_far(const float* __restrict__ x, int n) {
    float best = x[0];
    int arg = 0, c = 1;
    auto take = [&](float v, int at) {
        if (v > best || (v != v && best == best)) {
            best = v;
            arg = at;
        }
    };
    for (; c + 8 <= n; c += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = x[c + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) take(v[k], c + k);
    }
    if (c + 4 <= n) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = x[c + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) take(v[k], c + k);
        c += 4;
    }
    for (; c < n; ++c) take(x[c], c);
    return arg;
}

// Tile t = pairs [t P, min(NN, (t + 1) P)): its floats as aligned float4s q0 + tid + 256 k.  `origin` = the molecule's
// block moved down by `mis` floats to a 16-byte boundary; a float4 that is not wholly inside the block (the first and the
// last of a molecule) is read element by element, so no load leaves the tensor.
__device__ __forceinline__ void fetch_tile(const float* __restrict__ origin, int mis, int total, int E, int P, int NN, int t,
                                           int tid, float4 (&r)[4]) {
    const int p0 = t * P, p1 = min(NN, p0 + P);
    const int q0 = (p0 * E + mis) >> 2, q1 = (p1 * E + mis + 3) >> 2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = q0 + tid + k * DGR_THREADS;
        if (q >= q1) continue;
        const int e = 4 * q;
        if (e >= mis && e + 4 <= mis + total) {
            r[k] = ld4_stream(origin + e);
        } else {
            float v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = (e + c >= mis && e + c < mis + total) ? origin[e + c] : 0.0f;
            r[k] = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

__global__ __launch_bounds__(DGR_THREADS) void decode_graph_kernel(
    const float* __restrict__ node, const float* __restrict__ edge, const unsigned char* __restrict__ order2, int N, int M,
    int E, int cap, unsigned char* __restrict__ atoms, uchar4* __restrict__ bonds, int* __restrict__ n_bonds,
    unsigned char* __restrict__ component, int* __restrict__ n_components, int* __restrict__ largest,
    int* __restrict__ largest_size, unsigned short* __restrict__ valence2) {
    extern __shared__ __align__(16) unsigned char dgr_dyn[];
    float* stage = reinterpret_cast<float*>(dgr_dyn);               // DGR_STAGE_F4 float4
    unsigned char* lab = dgr_dyn + DGR_STAGE_F4 * 16;               // packed lower triangle of the bond labels
    __shared__ unsigned adj[DGR_WORDS * 256];                       // adj[w * 256 + i]: bits 32 w .. 32 w + 31 of atom i's row
    __shared__ int comp[256], rowoff[256], csize[256], wsum[4], best_key, ncomp;
    __shared__ unsigned char ord[256];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t b = blockIdx.x;
    const int NN = N * N, total = NN * E;
    const float* mol = edge + b * total;
    const int mis = static_cast<int>((reinterpret_cast<uintptr_t>(mol) >> 2) & 3);
    const float* origin = mol - mis;
    const int P = DGR_PAIR_FLOATS / E, ntiles = (NN + P - 1) / P;

    float4 r[4];
    fetch_tile(origin, mis, total, E, P, NN, 0, tid, r);
    for (int w = tid; w < DGR_WORDS * 256; w += DGR_THREADS) adj[w] = 0u;
    csize[tid] = 0;
    comp[tid] = tid;
    ord[tid] = (order2 && tid < E) ? order2[tid] : static_cast<unsigned char>(0);
    if (tid == 0) {
        best_key = 0;
        ncomp = 0;
    }
    if (tid < N) atoms[b * N + tid] = static_cast<unsigned char>(first_max_far(node + (b * N + tid) * M, M));
    __syncthreads();

    // ---- labels of the pairs i > j, adjacency bits ----
    for (int t = 0; t < ntiles; ++t) {
        const int p0 = t * P, p1 = min(NN, p0 + P);
        const int q0 = (p0 * E + mis) >> 2, q1 = (p1 * E + mis + 3) >> 2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = tid + k * DGR_THREADS;
            if (q0 + q < q1) st4(stage + 4 * q, r[k]);
        }
        __syncthreads();
        if (t + 1 < ntiles) fetch_tile(origin, mis, total, E, P, NN, t + 1, tid, r);
        for (int p = p0 + tid; p < p1; p += DGR_THREADS) {
            const int i = p / N, j = p - i * N;
            if (j >= i) continue;                                   // diagonal and upper triangle: never read by the decoder
            const int l = first_max(stage + (p * E + mis - 4 * q0), E);
            lab[tri(i) + j] = static_cast<unsigned char>(l);
            if (l) {
                atomicOr(&adj[(j >> 5) * 256 + i], 1u << (j & 31));
                atomicOr(&adj[(i >> 5) * 256 + j], 1u << (i & 31));
            }
        }
        __syncthreads();
    }

    // ---- ordered bond list: row counts, exclusive scan over the rows, prefix writes ----
    int cnt = 0;
    if (tid < N) {
#pragma unroll
        for (int w = 0; w < DGR_WORDS; ++w) {
            const unsigned word = adj[w * 256 + tid];
            const int lo = 32 * w;
            if (lo + 32 <= tid) cnt += __popc(word);
            else if (lo < tid) cnt += __popc(word & ((1u << (tid - lo)) - 1u));
        }
    }
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wv; ++w) before += wsum[w];
    rowoff[tid] = before + incl - cnt;
    if (tid == 0) n_bonds[b] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    for (int i = wv; i < N; i += DGR_THREADS / 64) {               // one wave per row, 64 candidate partners per step
        int base = rowoff[i];
        for (int c = 0; 64 * c < i; ++c) {
            unsigned long long m = static_cast<unsigned long long>(adj[(2 * c) * 256 + i]) |
                                   (static_cast<unsigned long long>(adj[(2 * c + 1) * 256 + i]) << 32);
            if (64 * (c + 1) > i) m &= (1ull << (i - 64 * c)) - 1ull;   // partners below i only (1 <= i - 64 c <= 63)
            if (m == 0ull) continue;
            if ((m >> lane) & 1ull) {
                const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
                const int j = 64 * c + lane;
                if (pos < cap)
                    bonds[b * cap + pos] = make_uchar4(static_cast<unsigned char>(i), static_cast<unsigned char>(j),
                                                       lab[tri(i) + j], 0);
            }
            base += __popcll(m);
        }
    }

    // ---- twice the valence: sum of order2[label] over the bonds of atom i ----
    if (valence2 && tid < N) {
        unsigned sum = 0;
        for (int w = 0; w < DGR_WORDS; ++w) {
            unsigned word = adj[w * 256 + tid];
            while (word) {
                const int k = 32 * w + __ffs(word) - 1;
                word &= word - 1u;
                const int hi = max(tid, k), lo = min(tid, k);
                sum += ord[lab[tri(hi) + lo]];
            }
        }
        valence2[b * N + tid] = static_cast<unsigned short>(sum);   // <= 255 partners x 255
    }

    // ---- connected components: synchronous min-label propagation with one pointer jump per round.  Labels only fall and
    // are always members of the atom's component, so the fixed point (the smallest index of the component) is unique; plain
    // propagation alone reaches it within N - 1 rounds, which bounds the loop. ----
    for (int round = 0; round < N; ++round) {
        int m = tid;
        if (tid < N) {
            m = comp[tid];
            for (int w = 0; w < DGR_WORDS; ++w) {
                unsigned word = adj[w * 256 + tid];
                while (word) {
                    const int k = 32 * w + __ffs(word) - 1;
                    word &= word - 1u;
                    m = min(m, comp[k]);
                }
            }
            m = min(m, comp[m]);
        }
        const int changed = __syncthreads_or(tid < N && m != comp[tid]);      // every read of this round is done
        if (!changed) break;
        if (tid < N) comp[tid] = m;
        __syncthreads();
    }
    if (tid < N) {
        const int c = comp[tid];
        component[b * N + tid] = static_cast<unsigned char>(c);
        atomicAdd(&csize[c], 1);
        if (c == tid) atomicAdd(&ncomp, 1);
    }
    __syncthreads();
    if (tid < N && comp[tid] == tid) atomicMax(&best_key, csize[tid] * 256 + (255 - tid));   // ties: the smaller label
    __syncthreads();
    if (tid == 0) {
        n_components[b] = ncomp;
        largest[b] = 255 - (best_key & 255);
        largest_size[b] = best_key >> 8;
    }
}

}  // namespace
}  // namespace dg

using namespace dg;

extern "C" int dg_decode_graph(const float* node_logits, const float* edge_logits, const unsigned char* order2, int B, int N,
                               int M, int E, int cap, unsigned char* atoms, unsigned char* bonds, int* n_bonds,
                               unsigned char* component, int* n_components, int* largest, int* largest_size,
                               unsigned short* valence2, dg_stream_t stream_) {
    if (!node_logits || !edge_logits || !atoms || !n_bonds || !component || !n_components || !largest || !largest_size)
        return fail(DG_E_ARG, "dg_decode_graph: null pointer");
    if (valence2 && !order2) return fail(DG_E_ARG, "dg_decode_graph: valence2 needs the order2 table");
    if (B < 0 || N < 1 || N > 256 || M < 1 || M > 255 || E < 1 || E > 255 || cap < 0)
        return fail(DG_E_SHAPE, "dg_decode_graph: need B >= 0, 1 <= N <= 256, 1 <= M, E <= 255, cap >= 0 (B=%d N=%d M=%d E=%d cap=%d)",
                    B, N, M, E, cap);
    if (cap > 0 && !bonds) return fail(DG_E_ARG, "dg_decode_graph: null pointer (bonds with cap > 0)");
    if ((reinterpret_cast<uintptr_t>(edge_logits) & 3) || (reinterpret_cast<uintptr_t>(bonds) & 3))
        return fail(DG_E_ARG, "dg_decode_graph: edge_logits and bonds must be 4-byte aligned");
    if (B == 0) return 0;
    const int tri_bytes = (N * (N - 1) / 2 + 15) & ~15;
    const size_t lds = static_cast<size_t>(DGR_STAGE_F4) * 16 + tri_bytes;      // <= 48 KiB: no opt-in needed
    hipLaunchKernelGGL(decode_graph_kernel, dim3(static_cast<unsigned>(B)), dim3(DGR_THREADS), lds,
                       static_cast<hipStream_t>(stream_), node_logits, edge_logits, order2, N, M, E, cap, atoms,
                       reinterpret_cast<uchar4*>(bonds), n_bonds, component, n_components, largest, largest_size, valence2);
    return check_launch("dg_decode_graph");
}
