// What the molecule kernels share (mol_stats.hip, mol_canon.hip): the 64-bit hash their keys are sums of, the wave sums, and
// the byte comparison that every key match has to pass.
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

}  // namespace dg
