// The ring notion of include/druggen_hip_fp.h, shared by mol_fp.hip and mol_valid.hip: a bond is in a ring when it is not a
// bridge of the graph of the bonds.  A breadth-first forest over the bonded atoms, then every bond outside the forest covers the
// two tree paths from its ends to their common ancestor: a tree bond is a bridge exactly when nothing covers it.  Both functions
// are called by the whole workgroup (they hold barriers), one thread per atom, N <= 256.
#pragma once

#include "common.h"

namespace dg {

constexpr int RING_NONE = 0xFFFF;                                // no parent

// words of a bit row in LDS: odd, so that the rows of neighbouring atoms start on different banks
__host__ __device__ constexpr int row_stride(int N) { return ((N + 31) >> 5) | 1; }

// The forest: one level, or one new root, per turn (at most 2 N turns).  adj: bit rows of row_stride(N) words; deg: the number
// of bonds per atom; bonded, front, vis: 8 words each, bonded = the atoms with deg > 0, front and vis zero on entry.  parent
// (RING_NONE on entry) and depth (0) are final on return.
__device__ __forceinline__ void ring_forest(int N, const unsigned* adj, const unsigned* deg, const unsigned* bonded, unsigned* front,
                                            unsigned* vis, unsigned short* parent, unsigned short* depth) {
    const int tid = threadIdx.x, W = (N + 31) >> 5, S = row_stride(N);
    for (int turn = 0; turn < 2 * N + 2; ++turn) {
        __syncthreads();                                            // front and vis are final
        bool any_front = false;
        int first = -1;                                             // the smallest bonded atom not reached yet
        for (int w = W - 1; w >= 0; --w) {
            any_front |= front[w] != 0u;
            const unsigned open = bonded[w] & ~vis[w];
            if (open) first = 32 * w + __ffs(open) - 1;
        }
        if (first < 0) break;                                       // (every thread read the same words)
        bool take = false;
        int par = RING_NONE, dep = 0;
        if (tid < N && deg[tid] && !((vis[tid >> 5] >> (tid & 31)) & 1u)) {
            if (!any_front) {
                take = tid == first;
            } else {
                for (int w = 0; w < W; ++w) {
                    const unsigned hit = adj[tid * S + w] & front[w];
                    if (hit) {
                        par = 32 * w + __ffs(hit) - 1;
                        dep = depth[par] + 1;
                        take = true;
                        break;
                    }
                }
            }
        }
        __syncthreads();                                            // everyone has read front and vis
        if (tid < 8) front[tid] = 0u;
        __syncthreads();
        if (take) {
            parent[tid] = static_cast<unsigned short>(par);
            depth[tid] = static_cast<unsigned short>(dep);
            atomicOr(&front[tid >> 5], 1u << (tid & 31));
            atomicOr(&vis[tid >> 5], 1u << (tid & 31));
        }
    }
    __syncthreads();
}

// The cover: cov[x] = 1 when the bond from x to parent[x] is on a cycle; ring (may be nullptr): the ends of every bond outside
// the forest.  list: the first `kept` rows (hi, lo, label, 0) of the molecule's bond list, of which those with both ends members
// count.  cov and ring are zero on entry and final after the caller's next barrier.
__device__ __forceinline__ void ring_cover(int N, const unsigned* __restrict__ list, int kept, const unsigned char* member,
                                           const unsigned short* parent, const unsigned short* depth, unsigned char* cov,
                                           unsigned char* ring) {
    for (int k = threadIdx.x; k < kept; k += blockDim.x) {
        const unsigned row = list[k];
        const int i = row & 255u, j = (row >> 8) & 255u;
        if (i >= N || j >= N || i == j || !member[i] || !member[j]) continue;
        if (parent[i] == j || parent[j] == i) continue;             // a tree bond
        if (ring) ring[i] = ring[j] = 1;
        int u = i, v = j;
        for (int step = 0; step < 2 * N && u != v; ++step) {        // the deeper end climbs
            int& up = depth[u] >= depth[v] ? u : v;
            const int p = parent[up];
            if (p == RING_NONE) break;                              // (the ends of a bond share a tree)
            cov[up] = 1;
            up = p;
        }
    }
}

}  // namespace dg
