// Canonical forms of a decoded batch (dg_mol_canon / dg_mol_canon_match of include/druggen_hip.h): an
// identity of a molecule that does not depend on the order of its atoms, for the reference's Uniqueness and Novelty curves
// (src/util/utils.py:241-355) without the host.  Colour refinement with hashed neighbour sums, individualisation of the
// smallest shared cell until the colouring is a bijection, then the graph rewritten in rank order.  Integers only; the only
// atomics are integer LDS adds / ors / mins; every loop carries its trip limit, nothing waits on another workgroup.
//
//   mol_canon_kernel    one workgroup of 256 lanes per molecule.  The atoms of the scope are compacted (lane m owns the m-th
//                       of them, ascending in position), the bonds between them live in LDS the way the decode keeps them:
//                       bit rows (word-major: lane m reads word w of its row without bank conflicts) and the packed lower
//                       triangle of labels.  A round is a walk over the set bits of the lane's row (mix64 per neighbour) and a
//                       rank count: n broadcast reads of (c, sig) per lane.
//   canon_match_rows    one workgroup per form b: the key scan of mol_key.h over j < b, then a binary search of the
//                       sorted stock keys and the same scan over the run of equal keys; every key match is verified byte by byte
//   canon_match_totals  one workgroup: tot[8]
#include <climits>

#include "common.h"
#include "mol_key.h"

namespace dg {
namespace {

constexpr int MCN_THREADS = MOL_THREADS;
constexpr int MCN_WORDS = 8;                                 // 32-bit words of a bit row (N <= 256)

__device__ __forceinline__ int tri(int i) { return (i * (i - 1)) >> 1; }      // offset of row i in the packed lower triangle

__global__ __launch_bounds__(MCN_THREADS) void mol_canon_kernel(
    const unsigned char* __restrict__ atoms, const unsigned* __restrict__ bonds, const int* __restrict__ n_bonds,
    const unsigned char* __restrict__ component, const int* __restrict__ largest, int N, int cap, int scope,
    int* __restrict__ out_n_atoms, int* __restrict__ out_n_bonds, int* __restrict__ out_n_splits, int* __restrict__ out_n_rounds,
    unsigned char* __restrict__ order, unsigned char* __restrict__ canon_atoms, unsigned* __restrict__ canon_bonds,
    unsigned long long* __restrict__ key) {
    extern __shared__ __align__(16) unsigned char lab[];            // bond labels between compact atoms hi > lo: lab[tri(hi) + lo]
    __shared__ unsigned adj[MCN_WORDS * 256];                       // adj[w * 256 + m]: bits 32 w .. 32 w + 31 of compact atom m's row
    __shared__ unsigned long long sig[256];
    __shared__ unsigned long long hkey;
    __shared__ int c[256], rowoff[256], touched[256], wsum[4], wsum2[4], pick, bonds_in;
    __shared__ unsigned short cidx[256];                            // position -> compact index, 0xFFFF: not in the scope
    __shared__ unsigned char pos[256], lab_a[256], inv[256];        // compact index -> position, -> atom label; rank -> compact index

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t b = blockIdx.x;
    unsigned char* ord_row = order + b * N;
    unsigned char* ca_row = canon_atoms + b * N;
    unsigned* cb_row = canon_bonds + b * cap;
    const int nb = n_bonds[b];
    if (nb > cap) {                                                 // truncated: its list is incomplete (uniform over the workgroup)
        if (tid < N) ord_row[tid] = ca_row[tid] = 0xFF;
        for (int k = tid; k < cap; k += MCN_THREADS) cb_row[k] = 0u;
        if (tid == 0) {
            out_n_atoms[b] = out_n_bonds[b] = out_n_rounds[b] = 0;
            out_n_splits[b] = -2;
            key[b] = 0ull;
        }
        return;
    }
    const int kept = max(nb, 0);
    const unsigned* list = bonds + b * cap;

    for (int w = tid; w < MCN_WORDS * 256; w += MCN_THREADS) adj[w] = 0u;
    touched[tid] = 0;
    if (tid == 0) {
        pick = INT_MAX;
        hkey = 0ull;
        bonds_in = 0;
    }
    __syncthreads();

    // ---- the scope: S, compacted in ascending position ----
    const unsigned a = tid < N ? atoms[b * N + tid] : 0u;
    if (scope == DG_CANON_WHOLE) {
        for (int k = tid; k < kept; k += MCN_THREADS) {
            const unsigned row = list[k];
            const int i = row & 255u, j = (row >> 8) & 255u;
            if (i < N && j < N && i != j) touched[i] = touched[j] = 1;
        }
        __syncthreads();
    }
    const bool member = tid < N && (scope == DG_CANON_LARGEST ? component[b * N + tid] == largest[b] : (a != 0u || touched[tid]));
    const unsigned long long mset = __ballot(member);
    if (lane == 0) wsum[wv] = __popcll(mset);
    __syncthreads();
    int first = 0;
    for (int w = 0; w < wv; ++w) first += wsum[w];
    const int n = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const int me = first + __popcll(mset & ((1ull << lane) - 1ull));
    cidx[tid] = member ? static_cast<unsigned short>(me) : static_cast<unsigned short>(0xFFFF);
    if (member) {
        pos[me] = static_cast<unsigned char>(tid);
        lab_a[me] = static_cast<unsigned char>(a);
    }
    __syncthreads();

    // ---- the bonds inside S ----
    for (int k = tid; k < kept; k += MCN_THREADS) {
        const unsigned row = list[k];
        const int i = row & 255u, j = (row >> 8) & 255u;
        if (i >= N || j >= N || i == j) continue;                   // (the decode never lists such a row)
        const int mi = cidx[i], mj = cidx[j];
        if (mi == 0xFFFF || mj == 0xFFFF) continue;
        const int hi = max(mi, mj), lo = min(mi, mj);
        lab[tri(hi) + lo] = static_cast<unsigned char>(row >> 16);
        atomicOr(&adj[(lo >> 5) * 256 + hi], 1u << (lo & 31));
        atomicOr(&adj[(hi >> 5) * 256 + lo], 1u << (hi & 31));
    }
    __syncthreads();

    // from here lane m < n owns compact atom m
    const bool on = tid < n;
    const int W = (n + 31) >> 5;
    {
        int cnt = 0;
        if (on) {
            for (int w = 0; w < W; ++w) {
                const unsigned word = adj[w * 256 + tid];
                const int lo = 32 * w;
                if (lo + 32 <= tid) cnt += __popc(word);
                else if (lo < tid) cnt += __popc(word & ((1u << (tid - lo)) - 1u));
            }
        }
        cnt = wave_sum(cnt);
        if (lane == 0) atomicAdd(&bonds_in, cnt);
    }

    // ---- start: c = count of atoms with a strictly smaller label ----
    {
        const unsigned mine = on ? lab_a[tid] : 0u;
        int less = 0;
        for (int j = 0; j < n; ++j) less += lab_a[j] < mine;
        c[tid] = less;
    }
    __syncthreads();

    // ---- refine; while a value of c is shared, individualise and refine again ----
    int splits = 0, rounds = 0;
    for (int pass = 0; pass < n; ++pass) {                          // a pass starts with at least pass + 1 cells
        int eq = 1;
        for (int r = 0; r < n; ++r) {                               // a round that changes c adds a cell
            if (on) {
                unsigned long long s = 0ull;
                for (int w = 0; w < W; ++w) {
                    unsigned word = adj[w * 256 + tid];
                    while (word) {
                        const int k = 32 * w + __ffs(word) - 1;
                        word &= word - 1u;
                        const unsigned l = lab[tri(max(tid, k)) + min(tid, k)];
                        s += mix64(static_cast<unsigned long long>(l << 16 | static_cast<unsigned>(c[k])));
                    }
                }
                sig[tid] = s;
            }
            __syncthreads();
            int less = 0;
            eq = 0;
            if (on) {
                const int cm = c[tid];
                const unsigned long long sm = sig[tid];
                for (int j = 0; j < n; ++j) {                       // every lane reads the same address: a broadcast
                    const int cj = c[j];
                    const unsigned long long sj = sig[j];
                    less += cj < cm || (cj == cm && sj < sm);
                    eq += cj == cm && sj == sm;
                }
            }
            ++rounds;
            const int changed = __syncthreads_or(on && less != c[tid]);      // every read of this round is done
            if (!changed) break;
            if (on) c[tid] = less;
            __syncthreads();
        }
        if (on && eq > 1) atomicMin(&pick, c[tid] << 8 | tid);      // the smallest shared value, its atom of smallest position
        __syncthreads();
        const int p = pick;
        if (p == INT_MAX) break;                                    // c is a bijection
        __syncthreads();
        if (tid == 0) pick = INT_MAX;
        if (on && c[tid] == (p >> 8) && tid != (p & 255)) c[tid] += 1;
        ++splits;
        __syncthreads();
    }

    // ---- the form: atoms in rank order ----
    unsigned long long h = 0ull;
    if (on) {
        const int r = c[tid];
        inv[r] = static_cast<unsigned char>(tid);
        ord_row[r] = pos[tid];
        ca_row[r] = lab_a[tid];
        h += mix(r, lab_a[tid]);
    } else if (tid < N) {
        ord_row[tid] = ca_row[tid] = 0xFF;
    }
    __syncthreads();

    // ---- bond rows (hi rank, lo rank, label) ascending: row counts, exclusive scan over the ranks, prefix writes ----
    int cnt = 0;
    if (on) {
        const int m = inv[tid];
        for (int w = 0; w < W; ++w) {
            unsigned word = adj[w * 256 + m];
            while (word) {
                const int k = 32 * w + __ffs(word) - 1;
                word &= word - 1u;
                cnt += c[k] < tid;
            }
        }
    }
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wsum2[wv] = incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wv; ++w) before += wsum2[w];
    rowoff[tid] = before + incl - cnt;
    __syncthreads();
    for (int R = wv; R < n; R += MCN_THREADS / 64) {                // one wave per rank, 64 candidate partners per step
        const int m = inv[R];
        int base = rowoff[R];
        for (int c0 = 0; 64 * c0 < R; ++c0) {
            const int j = 64 * c0 + lane;
            int mj = 0;
            bool bonded = false;
            if (j < R) {
                mj = inv[j];
                bonded = (adj[(mj >> 5) * 256 + m] >> (mj & 31)) & 1u;
            }
            const unsigned long long mask = __ballot(bonded);
            if (bonded) {
                const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
                const unsigned l = lab[tri(max(m, mj)) + min(m, mj)];
                const unsigned row = static_cast<unsigned>(R) | static_cast<unsigned>(j) << 8 | l << 16;
                if (at < cap) cb_row[at] = row;
                h += mix(258u + at, row);
            }
            base += __popcll(mask);
        }
    }
    const int nb_in = bonds_in;
    for (int k = nb_in + tid; k < cap; k += MCN_THREADS) cb_row[k] = 0u;
    if (tid == 0) h += mix(256u, static_cast<unsigned>(n)) + mix(257u, static_cast<unsigned>(nb_in));
    h = wave_sum(h);
    if (lane == 0) atomicAdd(&hkey, h);
    __syncthreads();
    if (tid == 0) {
        out_n_atoms[b] = n;
        out_n_bonds[b] = nb_in;
        out_n_splits[b] = splits;
        out_n_rounds[b] = rounds;
        key[b] = hkey;
    }
}

__global__ __launch_bounds__(MCN_THREADS) void canon_match_rows(
    const long long* __restrict__ key, Forms mine_side, int N, const long long* __restrict__ stock_keys,
    const int* __restrict__ stock_index, Forms stock, int S, unsigned long long mask, int* __restrict__ match) {
    __shared__ int first_dup, first_hit;
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    int* out = match + static_cast<int64_t>(b) * 2;
    if (mine_side.n_splits[b] < 0) {                                // truncated (uniform over the workgroup)
        if (tid == 0) out[0] = out[1] = -2;
        return;
    }
    const int n = max(0, min(mine_side.n_atoms[b], N)), nb = max(0, mine_side.n_bonds[b]);
    const unsigned long long mine = static_cast<unsigned long long>(key[b]) & mask;
    const unsigned char* my_atoms = mine_side.atoms + static_cast<int64_t>(b) * N;
    const unsigned* my_bonds = mine_side.bonds + static_cast<int64_t>(b) * mine_side.cap;
    const int dup = scan_equal(mine_side, key, nullptr, 0, b, mask, mine, n, nb, my_atoms, my_bonds, mine_side.cap, N, &first_dup);
    int hit = -3;
    if (S > 0) {
        // the run of my key in the sorted stock keys (signed order, the mask applied to both sides)
        const long long want = static_cast<long long>(mine);
        int lo = 0, hi = S;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (static_cast<long long>(static_cast<unsigned long long>(stock_keys[mid]) & mask) < want) lo = mid + 1;
            else hi = mid;
        }
        const int p0 = lo;
        hi = S;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (static_cast<long long>(static_cast<unsigned long long>(stock_keys[mid]) & mask) <= want) lo = mid + 1;
            else hi = mid;
        }
        const int p1 = lo;
        const int at = scan_equal(stock, stock_keys, stock_index, p0, p1, mask, mine, n, nb, my_atoms, my_bonds, mine_side.cap, N,
                                  &first_hit);
        hit = at < p1 ? stock_index[at] : -1;
    }
    if (tid == 0) {
        out[0] = dup < b ? dup : -1;
        out[1] = hit;
    }
}

__global__ __launch_bounds__(MCN_THREADS) void canon_match_totals(const int* __restrict__ match, const int* __restrict__ n_splits,
                                                                  int B, long long* __restrict__ tot) {
    unsigned long long part[5] = {};              // tot[1 .. 5]
    for (int64_t b = threadIdx.x; b < B; b += MCN_THREADS) {
        const int dup = match[2 * b], hit = match[2 * b + 1], split = n_splits[b];
        part[0] += dup == -1;
        part[1] += hit >= 0;
        part[2] += hit == -1;
        part[3] += split < 0;
        part[4] += split == 0;
    }
    store_totals<8>(part, B, tot);
}

}  // namespace
}  // namespace dg

using namespace dg;

extern "C" int dg_mol_canon(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds,
                            const unsigned char* component, const int* largest, int B, int N, int cap, int scope, int* n_atoms,
                            int* n_bonds_in, int* n_splits, int* n_rounds, unsigned char* order, unsigned char* canon_atoms,
                            unsigned char* canon_bonds, int64_t* key, dg_stream_t stream_) {
    if (B < 0 || N < 1 || N > 256 || cap < 0)
        return fail(DG_E_SHAPE, "dg_mol_canon: need B >= 0, 1 <= N <= 256, cap >= 0 (B=%d N=%d cap=%d)", B, N, cap);
    if (scope != DG_CANON_WHOLE && scope != DG_CANON_LARGEST)
        return fail(DG_E_ARG, "dg_mol_canon: scope must be 0 (whole) or 1 (largest), got %d", scope);
    if (!atoms || !n_bonds || !component || !largest || !n_atoms || !n_bonds_in || !n_splits || !n_rounds || !order ||
        !canon_atoms || !key)
        return fail(DG_E_ARG, "dg_mol_canon: null pointer");
    if (cap > 0 && (!bonds || !canon_bonds)) return fail(DG_E_ARG, "dg_mol_canon: null pointer (bonds / canon_bonds with cap > 0)");
    if (misaligned(bonds, 4) || misaligned(canon_bonds, 4) || misaligned(n_bonds, 4) || misaligned(largest, 4) ||
        misaligned(n_atoms, 4) || misaligned(n_bonds_in, 4) || misaligned(n_splits, 4) || misaligned(n_rounds, 4) ||
        misaligned(key, 8))
        return fail(DG_E_ARG, "dg_mol_canon: bond rows and int arrays must be 4-byte, key 8-byte aligned");
    if (B == 0) return 0;
    const size_t lds = static_cast<size_t>((N * (N - 1) / 2 + 15) & ~15);      // the label triangle, <= 32 640 B
    hipLaunchKernelGGL(mol_canon_kernel, dim3(static_cast<unsigned>(B)), dim3(MCN_THREADS), lds,
                       static_cast<hipStream_t>(stream_), atoms, reinterpret_cast<const unsigned*>(bonds), n_bonds, component,
                       largest, N, cap, scope, n_atoms, n_bonds_in, n_splits, n_rounds, order, canon_atoms,
                       reinterpret_cast<unsigned*>(canon_bonds), reinterpret_cast<unsigned long long*>(key));
    return check_launch("dg_mol_canon");
}

extern "C" int dg_mol_canon_match(const int64_t* key, const int* n_atoms, const int* n_bonds_in, const int* n_splits,
                                  const unsigned char* canon_atoms, const unsigned char* canon_bonds, int B, int N, int cap,
                                  const int64_t* stock_keys, const int* stock_index, const int* stock_n_atoms,
                                  const int* stock_n_bonds_in, const int* stock_n_splits, const unsigned char* stock_atoms,
                                  const unsigned char* stock_bonds, int S, int stock_cap, int key_bits, int* match, int64_t* tot,
                                  dg_stream_t stream_) {
    if (B < 0 || S < 0 || N < 1 || N > 256 || cap < 0 || stock_cap < 0)
        return fail(DG_E_SHAPE, "dg_mol_canon_match: need B >= 0, S >= 0, 1 <= N <= 256, cap >= 0, stock_cap >= 0 (B=%d S=%d N=%d "
                    "cap=%d stock_cap=%d)", B, S, N, cap, stock_cap);
    if (key_bits < 1 || key_bits > 64)
        return fail(DG_E_ARG, "dg_mol_canon_match: key_bits must be in 1..64 (got %d)", key_bits);
    if (!tot || (B > 0 && (!key || !n_atoms || !n_bonds_in || !n_splits || !canon_atoms || !match)))
        return fail(DG_E_ARG, "dg_mol_canon_match: null pointer");
    if (B > 0 && cap > 0 && !canon_bonds) return fail(DG_E_ARG, "dg_mol_canon_match: null pointer (canon_bonds with cap > 0)");
    if (B > 0 && S > 0 && (!stock_keys || !stock_index || !stock_n_atoms || !stock_n_bonds_in || !stock_n_splits || !stock_atoms ||
                           (stock_cap > 0 && !stock_bonds)))
        return fail(DG_E_ARG, "dg_mol_canon_match: null pointer (stock)");
    if (misaligned(key, 8) || misaligned(stock_keys, 8) || misaligned(tot, 8) || misaligned(n_atoms, 4) ||
        misaligned(n_bonds_in, 4) || misaligned(n_splits, 4) || misaligned(canon_bonds, 4) || misaligned(stock_index, 4) ||
        misaligned(stock_n_atoms, 4) || misaligned(stock_n_bonds_in, 4) || misaligned(stock_n_splits, 4) ||
        misaligned(stock_bonds, 4) || misaligned(match, 4))
        return fail(DG_E_ARG, "dg_mol_canon_match: bond rows and int arrays must be 4-byte, keys and tot 8-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const unsigned long long mask = key_bits == 64 ? ~0ull : (1ull << key_bits) - 1ull;
    if (B > 0) {
        const Forms mine{n_atoms, n_bonds_in, n_splits, canon_atoms, reinterpret_cast<const unsigned*>(canon_bonds), cap};
        const Forms stock{stock_n_atoms, stock_n_bonds_in, stock_n_splits, stock_atoms,
                          reinterpret_cast<const unsigned*>(stock_bonds), stock_cap};
        hipLaunchKernelGGL(canon_match_rows, dim3(static_cast<unsigned>(B)), dim3(MCN_THREADS), 0, stream,
                           reinterpret_cast<const long long*>(key), mine, N, reinterpret_cast<const long long*>(stock_keys),
                           stock_index, stock, S, mask, match);
    }
    hipLaunchKernelGGL(canon_match_totals, dim3(1), dim3(MCN_THREADS), 0, stream, match, n_splits, B,
                       reinterpret_cast<long long*>(tot));
    return check_launch("dg_mol_canon_match");
}
