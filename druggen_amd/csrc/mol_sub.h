// The atom predicate and the bounded depth-first search of include/druggen_hip_sub.h, for mol_sub.hip.  Plain C++ over
// pointers, so that tests/mol_sub_harness.cpp can run both on the host.  The staged molecule: per atom one property word
// (sub_prop), one set word, a neighbour count <= 8 and eight entries `neighbour << 8 | kind` in ascending order.
#pragma once

namespace dg {

constexpr int SUB_MAX_ATOMS = 16, SUB_MAX_CLOSURES = 8, SUB_MAX_STEPS = 4096, SUB_NBR = 8, SUB_WORDS = 80;
constexpr int SUB_ATOM0 = 8, SUB_CLOSURE0 = 72;                  // first atom word, first closure word of a record
constexpr unsigned SUB_IN_SCOPE = 1u << 31, SUB_RINGED = 1u << 16;
enum { SUB_MISS = 0, SUB_MATCH = 1, SUB_OVER = -1 };

// h | deg << 4 | n2 << 10 | n3 << 13 | (na > 0) << 15 | ringed << 16 (set later, from the bonds) | r3 << 17 | in scope << 31
__host__ __device__ inline unsigned sub_prop(unsigned key) {
    const unsigned h = (key >> 8) & 15u, n1 = (key >> 12) & 15u, n2 = (key >> 16) & 7u, n3 = (key >> 19) & 3u,
                   na = (key >> 21) & 7u, r3 = (key >> 24) & 1u;
    return h | (n1 + n2 + n3 + na) << 4 | n2 << 10 | n3 << 13 | (na ? 1u << 15 : 0u) | r3 << 17 | SUB_IN_SCOPE;
}

// bit `v` of the low `width` bits of `mask`: a value past the width matches nothing
__host__ __device__ inline bool sub_bit(unsigned mask, unsigned width, unsigned v) { return v < width && ((mask >> v) & 1u); }

// the predicate of the atom whose four words start at `aw`, for an atom of property word `p` and set word `s`
__host__ __device__ inline bool sub_atom_ok(const unsigned* aw, unsigned p, unsigned s) {
    const unsigned w1 = aw[1], w2 = aw[2];
    return (p & SUB_IN_SCOPE) && (s & aw[0]) && sub_bit(w1, 9u, p & 15u) && sub_bit(w1 >> 16, 9u, (p >> 4) & 63u) &&
           sub_bit(w2, 5u, (p >> 10) & 7u) && sub_bit(w2 >> 8, 3u, (p >> 13) & 3u) && sub_bit(w2 >> 12, 2u, (p >> 15) & 1u) &&
           sub_bit(w2 >> 14, 2u, (p >> 16) & 1u) && sub_bit(w2 >> 16, 2u, (p >> 17) & 1u);
}

// is there a BOND x - y whose kind bit is in `mask`?  (x's list, at most 8 entries)
__host__ __device__ inline bool sub_bonded(const unsigned char* ncnt, const unsigned short* nbr, int x, int y, unsigned mask) {
    const int n = ncnt[x] < SUB_NBR ? ncnt[x] : SUB_NBR;
    for (int i = 0; i < n; ++i) {
        const unsigned e = nbr[x * SUB_NBR + i];
        if (static_cast<int>(e >> 8) == y && ((mask >> (e & 7u)) & 1u)) return true;
    }
    return false;
}

// The search for pattern `pat` anchored at atom a.  m[k * stride] and cur[k * stride], k < 16, are this search's own bytes
// (LDS on the device: a run-time depth indexes them).  *steps gets the step count.  Every loop carries its trip limit: an
// iteration of the outer loop either counts a step (at most SUB_MAX_STEPS of them) or goes back one atom, which it can do
// no more often than it went forward.
__host__ __device__ inline int sub_search(const unsigned* pat, const unsigned* prop, const unsigned* sets,
                                          const unsigned char* ncnt, const unsigned short* nbr, int a, unsigned char* m,
                                          unsigned char* cur, int stride, int* steps) {
    const unsigned head = pat[0];
    int n = head & 255u, nc = (head >> 8) & 255u;
    n = n < 1 ? 1 : n > SUB_MAX_ATOMS ? SUB_MAX_ATOMS : n;
    nc = nc > SUB_MAX_CLOSURES ? SUB_MAX_CLOSURES : nc;
    *steps = 1;
    if (!sub_atom_ok(pat + SUB_ATOM0, prop[a], sets[a])) return SUB_MISS;
    if (n == 1) return SUB_MATCH;
    m[0] = static_cast<unsigned char>(a);
    int k = 1, count = 1;
    cur[stride] = 0;
    for (int it = 0; it < 2 * SUB_MAX_STEPS + SUB_MAX_ATOMS; ++it) {
        const unsigned* aw = pat + SUB_ATOM0 + 4 * k;
        const int from = m[(aw[3] & 15u) * stride];
        const int c = cur[k * stride];
        const int have = ncnt[from] < SUB_NBR ? ncnt[from] : SUB_NBR;
        if (c >= have) {                                         // the candidates of k ran out
            if (--k == 0) break;
            continue;
        }
        cur[k * stride] = static_cast<unsigned char>(c + 1);
        if (++count >= SUB_MAX_STEPS) {
            *steps = count;
            return SUB_OVER;
        }
        const unsigned e = nbr[from * SUB_NBR + c];
        const int v = e >> 8;
        if (!(((aw[3] >> 8) >> (e & 7u)) & 1u)) continue;
        bool ok = true;
        for (int j = 0; j < k && j < SUB_MAX_ATOMS; ++j) ok = ok && m[j * stride] != v;
        if (!ok || !sub_atom_ok(aw, prop[v], sets[v])) continue;
        for (int i = 0; i < nc && ok; ++i) {
            const unsigned cw = pat[SUB_CLOSURE0 + i];
            if (static_cast<int>(cw & 15u) == k) ok = sub_bonded(ncnt, nbr, v, m[((cw >> 8) & 15u) * stride], (cw >> 16) & 255u);
        }
        if (!ok) continue;
        m[k * stride] = static_cast<unsigned char>(v);
        if (k == n - 1) {
            *steps = count;
            return SUB_MATCH;
        }
        ++k;
        cur[k * stride] = 0;
    }
    *steps = count;
    return SUB_MISS;
}

}  // namespace dg
