// What the two designs of the graph attention core share: attn_core.hip (one wave per row, N <= 96) and
// attn_core_long.hip (one workgroup per row, N <= 256).
//
//   s_ij = alpha q_i k_j (e_ij^2 + e_ij)     p_ij = softmax_j s_ij     o_i = sum_j p_ij v_j
//
// Here: the lane layout, the placement of workgroups on XCDs, the gate and the score, the second order's tangent and
// slot body, and the host side's argument checks and (dtype, lqs, jpl) -> instance dispatch.  Each kernel keeps its own
// memory traffic, softmax merge, scheduling barriers and stores.
#pragma once

#include "bf16.h"

#include <initializer_list>

namespace dg {

constexpr float kNegBig = -3.0e38f;

// thread = (phase, quad) of a THREADS-wide row team (64: one wave, 256: one workgroup): quad selects four channels of
// a QS-quad slice, phase the neighbours j = phase, phase + P, ... (JPL slots per thread).
template <int THREADS, int LQS, int JPL>
struct Lane {
    static constexpr int QS = 1 << LQS;         // quads per slice
    static constexpr int P = THREADS >> LQS;    // neighbour phases per team
    int quad, phase;
    bool cok;          // this lane's channels exist
    int c0;            // channel offset (clamped to 0 when !cok)
    unsigned off[JPL]; // element offset of (neighbour slot, channel) inside one [N,C] row block
    bool jok[JPL];     // slot holds a real neighbour
    __device__ __forceinline__ Lane(int tid, int slice, int N, int C) {
        quad = tid & (QS - 1);
        phase = tid >> LQS;
        const int cq = slice * QS + quad;
        cok = cq * 4 < C;
        c0 = cok ? cq * 4 : 0;
#pragma unroll
        for (int t = 0; t < JPL; ++t) {
            const int j = phase + t * P;
            jok[t] = j < N;
            off[t] = static_cast<unsigned>((jok[t] ? j : 0) * C + c0);   // clamped: loads stay in bounds, results are masked
        }
    }
};

// XCD-aware placement (speed only): workgroup -> (molecule, channel slice, row group), SL * G workgroups per molecule.
// Workgroup id -> XCD is round robin (id % 8), and each XCD has its own L2.  Every workgroup of a molecule gets the same
// residue mod 8 and consecutive ids in that XCD's dispatch order: the molecule's k, v rows are fetched from HBM once
// instead of once per XCD (PMC, forward: reads 1.30x -> ~1.0x of the algorithmic bytes), and the slices that share a
// cache line run at the same time behind one L2 -- with bf16 rows a 32-channel slice covers 64 of a line's 128 bytes,
// and the other half is then an L2 hit instead of a second HBM fetch.
// reverse (traversal.h): molecules in descending order; b -> 8 ceil(B / 8) - 1 - b keeps a molecule on one XCD.
// The caller returns when b >= B (workgroup-uniform).  The struct form wraps the out-parameter form: hipcc schedules the
// one-wave forward as before only around the latter, the one-workgroup kernels only around the former.
__device__ __forceinline__ void place(int SL, int G, int B, int reverse, int& b, int& slice, int& group) {
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per = SL * G;
    b = (slot / per) * 8 + xcd;
    slice = (slot % per) % SL;
    group = (slot % per) / SL;
    if (reverse) b = (B + 7) / 8 * 8 - 1 - b;
}

struct Place {
    int b, slice, group;
};
__device__ __forceinline__ Place place(int SL, int G, int B, int reverse) {
    Place p;
    place(SL, G, B, reverse, p.b, p.slice, p.group);
    return p;
}

// ------------------------------------------------------ per-slot arithmetic ----
// gate g(e) = e^2 + e, its derivative, and the score s = alpha q k g(e) (aq = alpha q).  The first-order slot bodies
// build on them in each kernel.
__device__ __forceinline__ float4 gate(float4 e) { return fma4(e, e, e); }
__device__ __forceinline__ float4 dgate(float4 e) { return fma4(f4(2.f), e, f4(1.f)); }
__device__ __forceinline__ float4 score(float4 aq, float4 kk, float4 e) { return aq * kk * gate(e); }

// Second order (closed form: tests/kernel_math.py::attn_core_bwd2).  Operands by value, parameters in the order of
// their first use, te converted where it is used: the wording under which every instance compiles as before.
// Tangent of s along (tq, tk, te); te as float4 or still packed (raw4<T>):
template <typename R>
__device__ __forceinline__ float4 bwd2_tangent(float alpha, float4 e, float4 qi, float4 kk, float4 tqi, float4 tkk,
                                               R te) {
    const float4 g = gate(e);
    const float4 g1 = dgate(e);
    return alpha * (g * fma4(tqi, kk, qi * tkk) + qi * kk * g1 * cvt_raw(te));
}
// One slot of a row: p = softmax weight, sd = the tangent above, wss = the adjoint of s from outside, and the row's
// abar = sum_j p wo v, mm = sum_j p sd, PB = sum_j p pbar.  Returns ge_ij and adds the slot's terms to gq_i (without
// its alpha), gk_j, gv_j.  (attn_core_long.hip's bf16 multi-slot instances allocate registers differently around the
// call: that kernel keeps its own copy of these lines.)
__device__ __forceinline__ float4 bwd2_slot(float4 woi, float4 vv, float4 e, float4 p, float4 abar, float4 wss, bool jok,
                                            float4 sd, float4 mm, float4 tvv, float4 PB, float4 te, float4 kk, float4 tkk,
                                            float4 aq, float alpha, float4 tqi, float4 qi, float4& gqa, float4& gkk,
                                            float4& gvv) {
    const float4 a = woi * vv;
    const float4 g = gate(e);
    const float4 g1 = dgate(e);
    float4 ds = fma4(p, a - abar, wss);
    if (!jok) ds = f4(0.f);
    const float4 pdot = p * (sd - mm);
    const float4 pbar = sd * (a - abar) - mm * a + woi * tvv;
    const float4 sbar = p * (pbar - PB);
    const float4 g1te = g1 * te;
    // gq_i += sbar alpha k g + ds alpha (tk g + k g1 te)
    gqa += sbar * kk * g + ds * fma4(tkk, g, kk * g1te);
    // gk_j += sbar alpha q g + ds alpha (tq g + q g1 te)
    gkk += sbar * aq * g + alpha * (ds * fma4(tqi, g, qi * g1te));
    gvv = fma4(pdot, woi, gvv);
    // ge = sbar alpha q k g1 + ds alpha (tq k g1 + q tk g1 + 2 q k te)
    return sbar * aq * kk * g1 + alpha * (ds * (g1 * fma4(tqi, kk, qi * tkk) + 2.f * (qi * kk * te)));
}

// ---------------------------------------------------------------- host side ----
// What an entry checks before it enqueues anything, one function per kind of operation: the pointers that must not be
// NULL, the dtype, the shape.  `name` is the entry's; `need` is what its shape message adds (" (need ...)" or "").
struct ShapeCheck {
    bool ok;
    int B, N, C;
    const char* need;
};
inline int check_args(const char* name, std::initializer_list<const void*> required, int dtype, const ShapeCheck& sh) {
    for (const void* p : required)
        if (!p) return fail(DG_E_ARG, "%s: null pointer", name);
    if (!dtype_ok(dtype)) return fail(DG_E_ARG, "%s: unknown dtype %d", name, dtype);
    if (!sh.ok) return fail(DG_E_SHAPE, "%s: unsupported shape B=%d N=%d C=%d%s", name, sh.B, sh.N, sh.C, sh.need);
    return 0;
}
// forward: s may be NULL (scores not wanted)
inline int check_fwd(const char* name, const void* q, const void* k, const void* v, const void* e, const void* o,
                     int dtype, const ShapeCheck& sh) {
    return check_args(name, {q, k, v, e, o}, dtype, sh);
}
// backward: ws (= zeros) and add_e may be NULL
inline int check_bwd(const char* name, const void* q, const void* k, const void* v, const void* e, const void* wo,
                     const void* dq, const void* dk, const void* dv, const void* de, int dtype, const ShapeCheck& sh) {
    return check_args(name, {q, k, v, e, wo, dq, dk, dv, de}, dtype, sh);
}
// backward of backward: ws, gws may be NULL
inline int check_bwd2(const char* name, const void* q, const void* k, const void* v, const void* e, const void* wo,
                      const void* tq, const void* tk, const void* tv, const void* te, const void* gq, const void* gk,
                      const void* gv, const void* ge, const void* gwo, int dtype, const ShapeCheck& sh) {
    return check_args(name, {q, k, v, e, wo, tq, tk, tv, te, gq, gk, gv, ge, gwo}, dtype, sh);
}

// what an entry picks for a shape: log2 of the quads per slice, slots per thread, channel slices
struct Geometry {
    int lqs, jpl, slices;
};

// (dtype, lqs, jpl) -> kernel instance.  A Shapes<Shape<LQS, JPL>...> list names what an entry instantiates;
// dispatch() calls launch(T(), Shape<LQS, JPL>()) for the listed shape that matches, T = float or bf16_t, and returns
// its status, or check_launch's when that is 0.  A geometry that is not listed launches nothing: DG_E_SHAPE.
template <int LQS_, int JPL_>
struct Shape {
    static constexpr int LQS = LQS_, JPL = JPL_;
};
template <typename... S>
struct Shapes {};
template <typename F, typename... S>
int dispatch(Shapes<S...>, const char* name, int dtype, int lqs, int jpl, F&& launch) {
    int st = 0;
    const bool listed = ((lqs == S::LQS && jpl == S::JPL &&
                          ((st = dtype == DG_DTYPE_BF16 ? launch(bf16_t(), S()) : launch(float(), S())), true)) || ...);
    if (!listed) return fail(DG_E_SHAPE, "%s: no kernel for lqs=%d jpl=%d", name, lqs, jpl);
    return st ? st : check_launch(name);
}

}  // namespace dg
