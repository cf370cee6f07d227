// The environment key of include/druggen_hip_desc.h and the search of its table, for mol_desc.hip.  Plain C++ over pointers, so
// that tests/mol_env_harness.cpp can run both on the host.
#pragma once

namespace dg {

constexpr int ENV_SEARCH = 13;                                   // halvings that empty a range of DG_DESC_MAX_ENV = 2^12 rows

// label | h << 8 | n1 << 12 | n2 << 16 | n3 << 19 | na << 21 | r3 << 24; a field past its width (the header shows that a valid
// molecule has none but na == 8, which reaches bit 24) is cut to h, n1, na < 16, n2 < 8, n3 < 4, so that bits 25..31 stay zero
__host__ __device__ inline unsigned env_key(unsigned label, unsigned h, unsigned n1, unsigned n2, unsigned n3, unsigned na,
                                            unsigned r3) {
    return (label & 255u) | (h & 15u) << 8 | (n1 & 15u) << 12 | (n2 & 7u) << 16 | (n3 & 3u) << 19 | (na & 15u) << 21 |
           (r3 & 1u) << 24;
}

// The row of `table` ([n_env,4] words, keys strictly ascending in word 0, 0 <= n_env <= 4096) whose key is `key`, or -1: the
// first row whose key is not below `key`, by halving [lo, hi) -- a range of n rows leaves at most n / 2, so 13 halvings empty it.
__host__ __device__ inline int env_find(const unsigned* table, int n_env, unsigned key) {
    int lo = 0, hi = n_env;
    for (int step = 0; step < ENV_SEARCH && lo < hi; ++step) {
        const int mid = (lo + hi) >> 1;
        if (table[4 * mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_env && table[4 * lo] == key ? lo : -1;
}

}  // namespace dg
