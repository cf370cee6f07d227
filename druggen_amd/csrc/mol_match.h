// A maximum matching of a general graph of at most 256 vertices and degree at most 7, run by ONE lane over arrays in LDS
// (mol_valid.hip): a greedy start, then one breadth-first search for an augmenting path per vertex still free,
// odd cycles contracted as they are met (Edmonds' blossom algorithm in its array form: match, par, base and a queue).  Plain
// C++ over pointers, so that a host program can run the same code.  Every loop carries a trip limit derived from N and every
// index is checked before it is used: a limit that is reached is a bug, never an access out of bounds.
#pragma once

namespace dg {

constexpr int MATCH_NONE = 0xFFFF;
constexpr int MATCH_DEG = 7;                                     // neighbours per vertex

struct MatchState {
    unsigned short *match, *par, *base, *queue;                     // N entries each; match and par MATCH_NONE, base[i] = i on entry
    unsigned char* used;                                            // in the queue of this search (zero on entry)
    unsigned* seen;                                                 // stamps of the walks below (zero on entry)
    const unsigned char* vertex;                                    // vertex[i] != 0: i is a vertex of the graph
    const unsigned char* nbr;                                       // nbr[i * MATCH_DEG + k], k < deg[i]
    const unsigned* deg;
    unsigned stamp;
    int N, qt;
};

#define DG_HD __host__ __device__ inline

// the base of the innermost blossom that holds both a and b: the first common vertex of their paths to the root
DG_HD int match_lca(MatchState& s, int a, int b) {
    const unsigned mark = ++s.stamp;
    for (int t = 0; t <= s.N; ++t) {
        a = s.base[a];
        s.seen[a] = mark;
        const int m = s.match[a];
        if (m == MATCH_NONE || s.par[m] == MATCH_NONE) break;       // the root
        a = s.par[m];
    }
    for (int t = 0; t <= s.N; ++t) {
        b = s.base[b];
        if (s.seen[b] == mark) return b;
        const int m = s.match[b];
        if (m == MATCH_NONE || s.par[m] == MATCH_NONE) break;
        b = s.par[m];
    }
    return b;
}

// from v up to the base b: mark the bases on the way (stamp `mark`) and point par along the cycle, so that the odd vertices of
// the blossom can be left in either direction
DG_HD void match_mark_path(MatchState& s, int v, int b, int child, unsigned mark) {
    for (int t = 0; t <= s.N && s.base[v] != b; ++t) {
        const int m = s.match[v];
        if (m == MATCH_NONE) break;
        s.seen[s.base[v]] = mark;
        s.seen[s.base[m]] = mark;
        s.par[v] = static_cast<unsigned short>(child);
        child = m;
        if (s.par[m] == MATCH_NONE) break;
        v = s.par[m];
    }
}

DG_HD void match_push(MatchState& s, int i) {
    s.used[i] = 1;
    if (s.qt < s.N) s.queue[s.qt++] = static_cast<unsigned short>(i);
}

// the free vertex at the end of an augmenting path from `root` (follow par and match back), or MATCH_NONE
DG_HD int match_find_path(MatchState& s, int root) {
    s.qt = 0;
    match_push(s, root);
    for (int qh = 0; qh < s.qt && qh < s.N; ++qh) {
        const int v = s.queue[qh];
        const int dv = s.deg[v] < MATCH_DEG ? static_cast<int>(s.deg[v]) : MATCH_DEG;
        for (int k = 0; k < dv; ++k) {
            const int to = s.nbr[v * MATCH_DEG + k];
            if (to >= s.N || s.base[v] == s.base[to] || s.match[v] == to) continue;
            const int mt = s.match[to];
            if (to == root || (mt != MATCH_NONE && s.par[mt] != MATCH_NONE)) {      // `to` is outer too: an odd cycle
                const int cb = match_lca(s, v, to);
                const unsigned mark = ++s.stamp;
                match_mark_path(s, v, cb, to, mark);
                match_mark_path(s, to, cb, v, mark);
                // every vertex of the search tree is in the queue or the mate of one that is
                const int end = s.qt;
                for (int q = 0; q < end; ++q) {
                    const int x = s.queue[q];
                    for (int e = 0; e < 2; ++e) {
                        const int i = e ? s.match[x] : x;
                        if (i == MATCH_NONE || s.seen[s.base[i]] != mark) continue;
                        s.base[i] = static_cast<unsigned short>(cb);
                        if (!s.used[i]) match_push(s, i);
                    }
                }
            } else if (s.par[to] == MATCH_NONE) {
                s.par[to] = static_cast<unsigned short>(v);
                if (mt == MATCH_NONE) return to;
                match_push(s, mt);
            }
        }
    }
    return MATCH_NONE;
}

// Fills s.match with a maximum matching and returns the number of vertices it leaves free.
DG_HD int match_maximum(MatchState& s) {
    const int N = s.N;
    for (int v = 0; v < N; ++v) {                                   // the greedy start
        if (!s.vertex[v] || s.match[v] != MATCH_NONE) continue;
        const int dv = s.deg[v] < MATCH_DEG ? static_cast<int>(s.deg[v]) : MATCH_DEG;
        for (int k = 0; k < dv; ++k) {
            const int u = s.nbr[v * MATCH_DEG + k];
            if (u < N && u != v && s.match[u] == MATCH_NONE) {
                s.match[v] = static_cast<unsigned short>(u);
                s.match[u] = static_cast<unsigned short>(v);
                break;
            }
        }
    }
    int free_left = 0;
    for (int root = 0; root < N; ++root) {                          // a vertex whose search fails stays free for good
        if (!s.vertex[root] || s.match[root] != MATCH_NONE) continue;
        int v = match_find_path(s, root);
        if (v == MATCH_NONE) ++free_left;
        for (int t = 0; t <= N && v != MATCH_NONE; ++t) {           // flip the path
            const int pv = s.par[v];
            if (pv == MATCH_NONE) break;
            const int next = s.match[pv];
            s.match[v] = static_cast<unsigned short>(pv);
            s.match[pv] = static_cast<unsigned short>(v);
            v = next;
        }
        // undo the search: what it wrote lies in the queue and in the mates of the queue, before or after the flip
        for (int q = 0; q < s.qt; ++q) {
            const int x = s.queue[q];
            for (int e = 0; e < 2; ++e) {
                const int i = e ? s.match[x] : x;
                if (i == MATCH_NONE) continue;
                s.used[i] = 0;
                s.par[i] = MATCH_NONE;
                s.base[i] = static_cast<unsigned short>(i);
            }
        }
    }
    return free_left;
}

#undef DG_HD

}  // namespace dg
