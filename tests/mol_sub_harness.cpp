// Runs csrc/mol_sub.h on the host, as one thread of mol_sub.hip does (tests/test_mol_sub_host.py builds this with
// -D__host__= -D__device__=).  stdin: any number of cases
//     N P                                  atoms, patterns
//     key set ringed cnt e * cnt           per atom: its key (4294967295: outside the scope), its set word, whether it has a
//                                          ring bond, and its cnt <= 8 entries `neighbour << 8 | kind` in ascending order
//     word * 80                            per pattern
// stdout: per case and per (pattern, scope atom), pattern-major, one line "p a verdict steps" (verdict 1 match, 0 none, -1 OVER).
// The images and cursors sit between guard bytes that are checked after every search.
#include <cstdio>
#include <vector>

#include "../druggen_amd/csrc/mol_sub.h"

int main() {
    int N, P;
    while (std::scanf("%d %d", &N, &P) == 2) {
        if (N < 1 || N > 256 || P < 0 || P > 1024) return 1;
        std::vector<unsigned> prop(256, 0u), sets(256, 0u);
        std::vector<unsigned char> ncnt(256, 0);
        std::vector<unsigned short> nbr(256 * dg::SUB_NBR, 0xFFFF);
        for (int a = 0; a < N; ++a) {
            unsigned key, set, ringed, cnt;
            if (std::scanf("%u %u %u %u", &key, &set, &ringed, &cnt) != 4 || cnt > static_cast<unsigned>(dg::SUB_NBR)) return 1;
            prop[a] = key == 0xFFFFFFFFu ? 0u : dg::sub_prop(key) | (ringed ? dg::SUB_RINGED : 0u);
            sets[a] = set;
            ncnt[a] = static_cast<unsigned char>(cnt);
            for (unsigned i = 0; i < cnt; ++i) {
                unsigned e;
                if (std::scanf("%u", &e) != 1) return 1;
                nbr[a * dg::SUB_NBR + i] = static_cast<unsigned short>(e);
            }
        }
        std::vector<unsigned> table(static_cast<size_t>(P) * dg::SUB_WORDS + 1, 0xDEADBEEFu);      // one word of guard behind it
        for (size_t w = 0; w < static_cast<size_t>(P) * dg::SUB_WORDS; ++w)
            if (std::scanf("%u", &table[w]) != 1) return 1;
        for (int p = 0; p < P; ++p)
            for (int a = 0; a < N; ++a) {
                if (!(prop[a] & dg::SUB_IN_SCOPE)) continue;
                unsigned char state[8 + 2 * dg::SUB_MAX_ATOMS + 8];
                for (unsigned char& s : state) s = 0xA5;
                int steps = 0;
                const int verdict = dg::sub_search(table.data() + static_cast<size_t>(p) * dg::SUB_WORDS, prop.data(), sets.data(),
                                                   ncnt.data(), nbr.data(), a, state + 8, state + 8 + dg::SUB_MAX_ATOMS, 1, &steps);
                for (int g = 0; g < 8; ++g)
                    if (state[g] != 0xA5 || state[8 + 2 * dg::SUB_MAX_ATOMS + g] != 0xA5) return 2;
                std::printf("%d %d %d %d\n", p, a, verdict, steps);
            }
        std::printf("end\n");
    }
    return 0;
}
