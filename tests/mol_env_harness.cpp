// Runs csrc/mol_env.h on the host, as one thread of mol_desc.hip does (tests/test_mol_desc_host.py builds this with
// -D__host__= -D__device__=).  stdin: any number of cases
//     n q          rows of the table, queries
//     key * n      the keys, strictly ascending (the table gets rows (key, 7 * k + 1, 0, 0))
//     query * q
// and, after a line "-1 p", p lines "label h n1 n2 n3 na r3".  stdout: per case one line of q row indices (-1: no row) followed by
// the value word of each hit (0 for a miss); per key line the packed key.
#include <cstdio>
#include <vector>

#include "../druggen_amd/csrc/mol_env.h"

int main() {
    int n, q;
    while (std::scanf("%d %d", &n, &q) == 2) {
        if (n < 0) {
            for (int k = 0; k < q; ++k) {
                unsigned f[7];
                for (unsigned& x : f)
                    if (std::scanf("%u", &x) != 1) return 1;
                std::printf("%u\n", dg::env_key(f[0], f[1], f[2], f[3], f[4], f[5], f[6]));
            }
            continue;
        }
        std::vector<unsigned> table(4 * static_cast<size_t>(n) + 4, 0xDEADBEEFu);      // one row of guard behind the table
        for (int k = 0; k < n; ++k) {
            if (std::scanf("%u", &table[4 * k]) != 1) return 1;
            table[4 * k + 1] = 7u * k + 1u;
            table[4 * k + 2] = table[4 * k + 3] = 0u;
        }
        for (int k = 0; k < q; ++k) {
            unsigned key;
            if (std::scanf("%u", &key) != 1) return 1;
            const int at = dg::env_find(table.data(), n, key);
            std::printf("%d %u ", at, at >= 0 ? table[4 * at + 1] : 0u);
        }
        std::printf("\n");
    }
    return 0;
}
