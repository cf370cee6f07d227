// What the molecule kernels share (mol_stats.hip, mol_canon.hip): the 64-bit hash their keys are sums of, the wave sums, the
// byte comparison that every key match has to pass, the duplicate scan around it and the tail of the totals kernels.
#pragma once

#include "common.h"

namespace dg {

// splitmix64's finaliser
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ... over (position, value): a key is the SUM of these over all positions modulo 2^64, so lanes hash in parallel and the
// order in which they add does not matter.
__device__ __forceinline__ unsigned long long mix(unsigned pos, unsigned value) {
    return mix64((static_cast<unsigned long long>(pos) + 1ull) << 32 | value);
}

__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// n_atoms atom bytes and n_rows 4-byte bond rows of two molecules, compared by the 64 lanes of one wave together (called in
// wave-uniform control flow; the answer is wave-uniform)
__device__ __forceinline__ bool same_rows(const unsigned char* __restrict__ pa, const unsigned char* __restrict__ qa,
                                          int n_atoms, const unsigned* __restrict__ pb, const unsigned* __restrict__ qb,
                                          int n_rows, int lane) {
    bool differ = false;
    for (int i = lane; i < n_atoms; i += 64) differ |= pa[i] != qa[i];
    if (__any(differ)) return false;
    for (int k0 = 0; k0 < n_rows; k0 += 64) {
        const int k = k0 + lane;
        if (__any(k < n_rows && pb[k] != qb[k])) return false;
    }
    return true;
}

constexpr int MOL_THREADS = 256;                                    // the workgroup of scan_equal and store_totals: four waves

// One side of a comparison: molecules in their original order, N atom bytes and `cap` 4-byte bond rows each.  n_atoms ==
// nullptr: every molecule has the caller's n atoms; n_splits == nullptr: none is refused (n_splits < 0 marks one without a form).
struct Forms {
    const int *n_atoms, *n_bonds, *n_splits;
    const unsigned char* atoms;
    const unsigned* bonds;
    int cap;
};

// The duplicate scan over the positions [p0, p1) of `o`: position p holds the key keys[p] of molecule index[p] (index ==
// nullptr: molecule p).  A wave scans 64 keys per step, its chunks in ascending order, and verifies the key matches of a chunk
// one after the other with all its lanes: its first verified match is its smallest, the smallest of the four waves is the
// answer.  Returns the smallest position with a molecule equal to mine (n atoms, nb bonds), p1 if there is none.  Called by the
// whole workgroup (it holds barriers); `first` is a shared word of its own.
__device__ __forceinline__ int scan_equal(const Forms& o, const long long* __restrict__ keys, const int* __restrict__ index,
                                          int p0, int p1, unsigned long long mask, unsigned long long mine, int n, int nb,
                                          const unsigned char* my_atoms, const unsigned* my_bonds, int my_cap, int N, int* first) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) *first = p1;
    __syncthreads();
    const int rows = min(nb, min(my_cap, o.cap));                   // (nb itself for molecules that are not truncated)
    for (int base = p0 + 64 * wv; base < p1; base += MOL_THREADS) {
        if (base > *static_cast<volatile int*>(first)) break;       // another wave already holds a smaller one (a hint only)
        const int p = base + lane;
        int idx = 0;
        bool cand = false;
        if (p < p1) {
            idx = index ? index[p] : p;
            cand = (static_cast<unsigned long long>(keys[p]) & mask) == mine && (!o.n_splits || o.n_splits[idx] >= 0) &&
                   (!o.n_atoms || o.n_atoms[idx] == n) && o.n_bonds[idx] == nb;
        }
        unsigned long long matches = __ballot(cand);
        bool found = false;
        while (matches && !found) {
            const int src = __ffsll(static_cast<long long>(matches)) - 1;
            matches &= matches - 1ull;
            const int64_t other = __shfl(idx, src, 64);
            found = same_rows(my_atoms, o.atoms + other * N, n, my_bonds, o.bonds + other * o.cap, rows, lane);
            if (found && lane == 0) atomicMin(first, base + src);
        }
        if (found) break;
    }
    __syncthreads();
    return *first;
}

// The tail of a totals kernel, entered by its one workgroup: tot[0] = B, tot[1 + k] = the sum of part[k] over the lanes,
// zeros from tot[1 + K] to tot[T - 1].
template <int T, int K>
__device__ __forceinline__ void store_totals(const unsigned long long (&part)[K], int B, long long* __restrict__ tot) {
    static_assert(K < T && T <= 64, "tot[0] is B; one lane per entry");
    __shared__ unsigned long long acc[T];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < T) acc[tid] = 0ull;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned long long s = wave_sum(part[k]);
        if (lane == 0) atomicAdd(&acc[k + 1], s);
    }
    __syncthreads();
    if (tid < T) tot[tid] = tid == 0 ? static_cast<long long>(B) : static_cast<long long>(acc[tid]);
}

}  // namespace dg
