// Host harness of csrc/mol_match.h for tests/test_mol_valid_host.py: reads graphs from stdin -- "n_slots n_edges", then n_slots
// vertex flags, then the edges -- runs match_maximum as the kernel's lane 0 does and prints, per graph, the number of vertices
// left free, whether the search state was left as it was found, and the mate of every slot (-1: none).
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../druggen_amd/csrc/mol_match.h"

int main() {
    int n, m;
    while (std::scanf("%d %d", &n, &m) == 2) {
        std::vector<unsigned char> vertex(n), used(n, 0), nbr(n * dg::MATCH_DEG, 0xEE);
        std::vector<unsigned> deg(n, 0), seen(n, 0);
        std::vector<unsigned short> match(n, dg::MATCH_NONE), par(n, dg::MATCH_NONE), base(n), queue(n, 0);
        std::vector<std::vector<int>> lists(n);
        for (int i = 0; i < n; ++i) {
            int flag;
            if (std::scanf("%d", &flag) != 1) return 2;
            vertex[i] = static_cast<unsigned char>(flag);
            base[i] = static_cast<unsigned short>(i);
        }
        for (int e = 0; e < m; ++e) {
            int a, b;
            if (std::scanf("%d %d", &a, &b) != 2) return 2;
            lists[a].push_back(b);
            lists[b].push_back(a);
        }
        for (int i = 0; i < n; ++i) {
            std::sort(lists[i].begin(), lists[i].end());
            if (lists[i].size() > static_cast<size_t>(dg::MATCH_DEG)) return 3;
            deg[i] = static_cast<unsigned>(lists[i].size());
            for (size_t k = 0; k < lists[i].size(); ++k) nbr[i * dg::MATCH_DEG + k] = static_cast<unsigned char>(lists[i][k]);
        }
        dg::MatchState s{match.data(), par.data(), base.data(), queue.data(), used.data(), seen.data(),
                         vertex.data(), nbr.data(), deg.data(), 0u, n, 0};
        const int free_left = dg::match_maximum(s);
        bool clean = true;
        for (int i = 0; i < n; ++i) clean &= !used[i] && par[i] == dg::MATCH_NONE && base[i] == i;
        std::printf("%d %d", free_left, clean ? 1 : 0);
        for (int i = 0; i < n; ++i) std::printf(" %d", match[i] == dg::MATCH_NONE ? -1 : static_cast<int>(match[i]));
        std::printf("\n");
    }
    return 0;
}
