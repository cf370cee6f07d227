// Graph attention core (reference src/model/layers.py:119-134) for long neighbour lists: 1 <= N <= 256.
// Forward, backward with the add_e adjoint, backward of backward.  The lane layout, the XCD-aware placement, the gate and
// the score, the second order's tangent, and the host side's argument checks and instance dispatch are csrc/attn_core.h,
// shared with attn_core.hip:
//
//   s_ij = alpha q_i k_j (e_ij^2 + e_ij)     p_ij = softmax_j s_ij     o_i = sum_j p_ij v_j
//
// attn_core.hip keeps every neighbour of a row in the lanes of ONE wave (12 slots x 8 phases = 96 at most).  Here a
// row is spread over a whole 256-thread workgroup:
//   * thread = (phase, quad): quad = tid & (QS-1) selects four channels of a QS-quad slice, phase = tid >> LQS selects
//     the neighbours j = phase, phase + P, ... (P = 256 / QS phases, JPL slots per thread).  Wide slices (forward,
//     backward): QS = 8 (32 channels, P = 32, JPL <= 8).  The second order carries five row tensors per slot and takes
//     QS = 4 (16 channels, P = 64, JPL <= 4); the two slices of a 128-byte line run next to each other on one XCD.
//   * a row's [N, slice] block of e (ws, te, add_e) is loaded once into registers: one HBM pass, no second read.
//   * the row reductions (softmax max / sum and every p-weighted sum the outputs need) are done per wave with the xor
//     butterfly, then merged across the four waves through LDS as online-softmax states (m_w, l_w, sum_w) in the fixed
//     order w = 0..3 -- one barrier per row.  The row sums that need the merged statistics first (dq, gq) are reduced
//     per wave and merged at the next row's barrier.
//   * k_j, v_j (tk_j, tv_j) and the column sums dk_j, dv_j (gk_j, gv_j) belong to fixed threads for the whole walk.  The
//     rows of a molecule are split over G row groups (workgroups); each writes its column sums to a float32 workspace
//     [2][G][B,N,C] and a second launch adds the G partials in ascending order.  No atomics: bit-reproducible in both
//     traversal directions.
#include "attn_core.h"
#include "traversal.h"

#include <type_traits>

namespace dg {
namespace {

constexpr int kThreads = 256;      // four waves per workgroup
constexpr int kFwdRows = 16;       // rows per forward workgroup: the k, v staging is 2/16 of the row traffic
constexpr int kBwdRows = 32;       // rows per backward workgroup: the column partials are 2/32 of a row tensor

// ---------------------------------------------------------------- forward ----
template <typename T, int LQS, int JPL>
__global__ __launch_bounds__(kThreads, 2) void attn_long_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                   const T* __restrict__ v, const T* __restrict__ e,
                                                                   T* __restrict__ s, T* __restrict__ o, int N, int C,
                                                                   float alpha, int SL, int G, int B, int reverse) {
    constexpr int QS = 1 << LQS;
    __shared__ float4 X[2][4][3][QS];    // per row parity and wave: (max, sum, sum p v)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const Place pl = place(SL, G, B, reverse);
    if (pl.b >= B) return;   // workgroup-uniform
    const int b = pl.b;
    const Lane<kThreads, LQS, JPL> L(tid, pl.slice, N, C);
    const size_t NC = static_cast<size_t>(N) * C;
    float4 kk[JPL], vv[JPL];
#pragma unroll
    for (int t = 0; t < JPL; ++t) {
        kk[t] = ld4(k + b * NC + L.off[t]);
        vv[t] = ld4(v + b * NC + L.off[t]);
    }
    const int R = (N + G - 1) / G, i0 = pl.group * R, i1 = min(N, i0 + R);
    typedef typename raw4<T>::type Raw;
    int par = 0;
    for (int i = i0; i < i1; ++i, par ^= 1) {
        const size_t row = static_cast<size_t>(b) * N + i;
        Raw re[JPL];
#pragma unroll
        for (int t = 0; t < JPL; ++t) re[t] = ld_raw_stream(e + row * NC + L.off[t]);
        const float4 aq = alpha * ld4(q + row * C + L.c0);
        T* sr = s + row * NC;
        float4 sv[JPL];
        float4 m = f4(kNegBig);
#pragma unroll
        for (int t = 0; t < JPL; ++t) {
            const float4 ee = cvt_raw(re[t]);
            sv[t] = score(aq, kk[t], ee);
            if (L.jok[t]) {
                m = max4(m, sv[t]);
                if (L.cok && s) st4_stream(sr + L.off[t], sv[t]);
            }
        }
        m = xor_max4<QS>(m);
        float4 l = f4(0.f), acc = f4(0.f);
#pragma unroll
        for (int t = 0; t < JPL; ++t) {
            const float4 pe = L.jok[t] ? exp4(sv[t] - m) : f4(0.f);
            l += pe;
            acc = fma4(pe, vv[t], acc);
        }
        l = xor_sum4<QS>(l);
        acc = xor_sum4<QS>(acc);
        if (lane < QS) {
            X[par][w][0][L.quad] = m;
            X[par][w][1][L.quad] = l;
            X[par][w][2][L.quad] = acc;
        }
        __syncthreads();
        // (X[par] is written again two rows later, after the next barrier: every reader has passed this one)
        if (tid < QS && L.cok) {
            float4 M = X[par][0][0][tid];
#pragma unroll
            for (int u = 1; u < 4; ++u) M = max4(M, X[par][u][0][tid]);
            float4 lt = f4(0.f), at = f4(0.f);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 f = exp4(X[par][u][0][tid] - M);
                lt = fma4(f, X[par][u][1][tid], lt);
                at = fma4(f, X[par][u][2][tid], at);
            }
            st4(o + row * C + L.c0, at * rcp4(lt));
        }
    }
}

// column sums of one row group: straight into (dk, dv) when there is one group, else into the float32 partials
template <typename T, int JPL, typename L_>
__device__ __forceinline__ void store_columns(const L_& L, const float4* a, const float4* c, T* ka, T* va, float* part,
                                              int b, int group, int G, int B, size_t NC) {
    const size_t BNC = static_cast<size_t>(B) * NC;
#pragma unroll
    for (int t = 0; t < JPL; ++t) {
        if (!(L.jok[t] && L.cok)) continue;
        const size_t at = b * NC + L.off[t];
        if (G == 1) {
            st4(ka + at, a[t]);
            st4(va + at, c[t]);
        } else {
            st4(part + group * BNC + at, a[t]);
            st4(part + (G + group) * BNC + at, c[t]);
        }
    }
}

// --------------------------------------------------------------- backward ----
// ADDE: `add_e` [B,N,N,C] is added to de on its way out (the gradient penalty's second-order adjoint of e, loss.py:32-47).
template <typename T, int LQS, int JPL, bool ADDE>
__global__ __launch_bounds__(kThreads, 2) void attn_long_bwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ e,
    const T* __restrict__ ws, const T* __restrict__ wo, const T* __restrict__ add_e, T* __restrict__ dq,
    T* __restrict__ dk, T* __restrict__ dv, T* __restrict__ de, float* __restrict__ part, int N, int C, float alpha,
    int SL, int G, int B, int reverse) {
    constexpr int QS = 1 << LQS;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float4* kv = reinterpret_cast<float4*>(smem_raw);             // [2][JPL][256]: k, v of this thread's slots
    float4(*X)[4][4][QS] = reinterpret_cast<float4(*)[4][4][QS]>(kv + 2 * JPL * kThreads);   // [2][4][(m, l, sum p v, dq)]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const Place pl = place(SL, G, B, reverse);
    if (pl.b >= B) return;   // workgroup-uniform
    const int b = pl.b;
    const Lane<kThreads, LQS, JPL> L(tid, pl.slice, N, C);
    const size_t NC = static_cast<size_t>(N) * C;
#pragma unroll
    for (int t = 0; t < JPL; ++t) {        // each thread reads back only its own entries: no barrier
        kv[(0 * JPL + t) * kThreads + tid] = ld4(k + b * NC + L.off[t]);
        kv[(1 * JPL + t) * kThreads + tid] = ld4(v + b * NC + L.off[t]);
    }
    float4 dkk[JPL], dvv[JPL];
#pragma unroll
    for (int t = 0; t < JPL; ++t) dkk[t] = dvv[t] = f4(0.f);
    const int R = (N + G - 1) / G, i0 = pl.group * R, i1 = min(N, i0 + R);
    typedef typename raw4<T>::type Raw;
    float4 dqp = f4(0.f);     // this wave's share of the previous row's dq
    int par = 0;
    for (int i = i0; i < i1; ++i, par ^= 1) {
        const size_t row = static_cast<size_t>(b) * N + i;
        Raw re[JPL], rws[JPL], rae[ADDE ? JPL : 1];
#pragma unroll
        for (int t = 0; t < JPL; ++t) {
            re[t] = ld_raw_stream(e + row * NC + L.off[t]);
            if (ws) rws[t] = ld_raw_stream(ws + row * NC + L.off[t]);
            if (ADDE) rae[ADDE ? t : 0] = ld_raw_stream(add_e + row * NC + L.off[t]);
        }
        const float4 aq = alpha * ld4(q + row * C + L.c0);
        const float4 woi = ld4(wo + row * C + L.c0);
        int kl = tid;                       // opaque per row: keeps the LDS operand reads inside the loop
        asm volatile("" : "+v"(kl));
        float4 pe[JPL];
        float4 m = f4(kNegBig);
#pragma unroll
        for (int t = 0; t < JPL; ++t) {
            const float4 ee = cvt_raw(re[t]);
            pe[t] = score(aq, kv[(0 * JPL + t) * kThreads + kl], ee);
            if (L.jok[t]) m = max4(m, pe[t]);
        }
        m = xor_max4<QS>(m);
        float4 l = f4(0.f), V = f4(0.f);
#pragma unroll
        for (int t = 0; t < JPL; ++t) {
            pe[t] = L.jok[t] ? exp4(pe[t] - m) : f4(0.f);
            l += pe[t];
            V = fma4(pe[t], kv[(1 * JPL + t) * kThreads + kl], V);
        }
        l = xor_sum4<QS>(l);
        V = xor_sum4<QS>(V);
        if (lane < QS) {
            X[par][w][0][L.quad] = m;
            X[par][w][1][L.quad] = l;
            X[par][w][2][L.quad] = V;
            X[par][w][3][L.quad] = dqp;
        }
        __syncthreads();
        if (tid < QS && i > i0 && L.cok) {    // previous row's dq: the four waves' shares in order
            float4 d = X[par][0][3][tid];
#pragma unroll
            for (int u = 1; u < 4; ++u) d += X[par][u][3][tid];
            st4(dq + (row - 1) * C + L.c0, alpha * d);
        }
        float4 M = X[par][0][0][L.quad];
#pragma unroll
        for (int u = 1; u < 4; ++u) M = max4(M, X[par][u][0][L.quad]);
        float4 lt = f4(0.f), vt = f4(0.f), fw = f4(0.f);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 f = exp4(X[par][u][0][L.quad] - M);
            lt = fma4(f, X[par][u][1][L.quad], lt);
            vt = fma4(f, X[par][u][2][L.quad], vt);
            if (u == w) fw = f;
        }
        const float4 inv = rcp4(lt);
        const float4 abar = woi * vt * inv;
        const float4 scale = fw * inv;        // p = pe * scale
        T* der = de + row * NC;
        float4 dqa = f4(0.f);
#pragma unroll
        for (int t = 0; t < JPL; ++t) {
            const float4 ee = cvt_raw(re[t]);
            const float4 kk = kv[(0 * JPL + t) * kThreads + kl];
            const float4 p = pe[t] * scale;
            float4 ds = fma4(p, woi * kv[(1 * JPL + t) * kThreads + kl] - abar, ws ? cvt_raw(rws[t]) : f4(0.f));
            if (!L.jok[t]) ds = f4(0.f);
            dvv[t] = fma4(p, woi, dvv[t]);
            const float4 dsg = ds * gate(ee);
            dqa = fma4(dsg, kk, dqa);
            dkk[t] = fma4(dsg, aq, dkk[t]);
            float4 dev = ds * aq * kk * dgate(ee);
            if (ADDE) dev += cvt_raw(rae[ADDE ? t : 0]);
            if (L.jok[t] && L.cok) st4_stream(der + L.off[t], dev);
        }
        dqp = xor_sum4<QS>(dqa);
    }
    if (i1 > i0) {     // the last row's dq
        if (lane < QS) X[par][w][3][L.quad] = dqp;
        __syncthreads();
        if (tid < QS && L.cok) {
            float4 d = X[par][0][3][tid];
#pragma unroll
            for (int u = 1; u < 4; ++u) d += X[par][u][3][tid];
            st4(dq + (static_cast<size_t>(b) * N + i1 - 1) * C + L.c0, alpha * d);
        }
    }
    store_columns<T, JPL>(L, dkk, dvv, dk, dv, part, b, pl.group, G, B, NC);
}

// ---------------------------------------------------- backward of backward ----
// Inputs of the first-order backward: (q,k,v,e,ws,wo); (tq,tk,tv,te) are the adjoints of its outputs (dq,dk,dv,de).
// Closed form: tests/kernel_math.py::attn_core_bwd2.  Every row sum is a p-weighted sum over j, so one merge carries
// them all: with pe = exp(s - m), l = sum pe, SV = sum pe v, SS = sum pe sd, SSV = sum pe sd v, STV = sum pe tv
//   abar = wo SV / l,  mm = SS / l,  gwo = (SSV - mm SV + STV) / l,
// and the slots take pbar_j - sum_j p pbar in its centred form (sd_j - mm)(a_j - abar) + wo (tv_j - gwo): each factor is
// one difference of like quantities.  (As pbar_j - [wo (SSV + STV) / l - 2 mm abar] the two sides round their mm a
// products apart, and where one neighbour holds the row's weight -- pbar_j = sum_j p pbar up to exp(-gap) -- that
// rounding was the whole result: gq, ge an order of magnitude above the one-wave kernel)
template <typename T, int LQS, int JPL>
__global__ __launch_bounds__(kThreads, 2) void attn_long_bwd2_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ e,
    const T* __restrict__ ws, const T* __restrict__ wo, const T* __restrict__ tq, const T* __restrict__ tk,
    const T* __restrict__ tv, const T* __restrict__ te, T* __restrict__ gq, T* __restrict__ gk, T* __restrict__ gv,
    T* __restrict__ ge, T* __restrict__ gws, T* __restrict__ gwo, float* __restrict__ part, int N, int C, float alpha,
    int SL, int G, int B, int reverse) {
    constexpr int QS = 1 << LQS;
    constexpr int NV = 7;      // m, l, SV, SS, SSV, STV, gq
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float4* kv = reinterpret_cast<float4*>(smem_raw);             // [4][JPL][256]: k, v, tk, tv of this thread's slots
    float4(*X)[4][NV][QS] = reinterpret_cast<float4(*)[4][NV][QS]>(kv + 4 * JPL * kThreads);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const Place pl = place(SL, G, B, reverse);
    if (pl.b >= B) return;   // workgroup-uniform
    const int b = pl.b;
    const Lane<kThreads, LQS, JPL> L(tid, pl.slice, N, C);
    const size_t NC = static_cast<size_t>(N) * C;
#pragma unroll
    for (int t = 0; t < JPL; ++t) {
        const size_t off = b * NC + L.off[t];
        kv[(0 * JPL + t) * kThreads + tid] = ld4(k + off);
        kv[(1 * JPL + t) * kThreads + tid] = ld4(v + off);
        kv[(2 * JPL + t) * kThreads + tid] = ld4(tk + off);
        kv[(3 * JPL + t) * kThreads + tid] = ld4(tv + off);
    }
    float4 gkk[JPL], gvv[JPL];
#pragma unroll
    for (int t = 0; t < JPL; ++t) gkk[t] = gvv[t] = f4(0.f);
    const int R = (N + G - 1) / G, i0 = pl.group * R, i1 = min(N, i0 + R);
    typedef typename raw4<T>::type Raw;
    float4 gqp = f4(0.f);
    int par = 0;
    for (int i = i0; i < i1; ++i, par ^= 1) {
        const size_t row = static_cast<size_t>(b) * N + i;
        Raw re[JPL], rws[JPL], rte[JPL];
#pragma unroll
        for (int t = 0; t < JPL; ++t) {
            re[t] = ld_raw_stream(e + row * NC + L.off[t]);
            if (ws) rws[t] = ld_raw_stream(ws + row * NC + L.off[t]);
            rte[t] = ld_raw_stream(te + row * NC + L.off[t]);
        }
        const float4 qi = ld4(q + row * C + L.c0);
        const float4 aq = alpha * qi;
        const float4 woi = ld4(wo + row * C + L.c0);
        const float4 tqi = ld4(tq + row * C + L.c0);
        int kl = tid;
        asm volatile("" : "+v"(kl));
        float4 pe[JPL], sd[JPL];
        float4 m = f4(kNegBig);
#pragma unroll
        for (int t = 0; t < JPL; ++t) {
            const float4 ee = cvt_raw(re[t]);
            pe[t] = score(aq, kv[(0 * JPL + t) * kThreads + kl], ee);
            if (L.jok[t]) m = max4(m, pe[t]);
        }
        m = xor_max4<QS>(m);
        float4 l = f4(0.f), SV = f4(0.f), SS = f4(0.f), SSV = f4(0.f), STV = f4(0.f);
        T* gwr = gws + row * NC;
#pragma unroll
        for (int t = 0; t < JPL; ++t) {
            const float4 ee = cvt_raw(re[t]);
            const float4 kk = kv[(0 * JPL + t) * kThreads + kl];
            const float4 vv = kv[(1 * JPL + t) * kThreads + kl];
            const float4 tkk = kv[(2 * JPL + t) * kThreads + kl];
            sd[t] = bwd2_tangent(alpha, ee, qi, kk, tqi, tkk, rte[t]);
            if (L.jok[t] && L.cok && gws) st4_stream(gwr + L.off[t], sd[t]);
            pe[t] = L.jok[t] ? exp4(pe[t] - m) : f4(0.f);
            const float4 ps = pe[t] * sd[t];
            l += pe[t];
            SV = fma4(pe[t], vv, SV);
            SS += ps;
            SSV = fma4(ps, vv, SSV);
            STV = fma4(pe[t], kv[(3 * JPL + t) * kThreads + kl], STV);
        }
        l = xor_sum4<QS>(l);
        SV = xor_sum4<QS>(SV);
        SS = xor_sum4<QS>(SS);
        SSV = xor_sum4<QS>(SSV);
        STV = xor_sum4<QS>(STV);
        if (lane < QS) {
            X[par][w][0][L.quad] = m;
            X[par][w][1][L.quad] = l;
            X[par][w][2][L.quad] = SV;
            X[par][w][3][L.quad] = SS;
            X[par][w][4][L.quad] = SSV;
            X[par][w][5][L.quad] = STV;
            X[par][w][6][L.quad] = gqp;
        }
        __syncthreads();
        if (tid < QS && i > i0 && L.cok) {    // previous row's gq
            float4 d = X[par][0][6][tid];
#pragma unroll
            for (int u = 1; u < 4; ++u) d += X[par][u][6][tid];
            st4(gq + (row - 1) * C + L.c0, alpha * d);
        }
        float4 M = X[par][0][0][L.quad];
#pragma unroll
        for (int u = 1; u < 4; ++u) M = max4(M, X[par][u][0][L.quad]);
        float4 lt = f4(0.f), svt = f4(0.f), sst = f4(0.f), ssvt = f4(0.f), stvt = f4(0.f), fw = f4(0.f);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 f = exp4(X[par][u][0][L.quad] - M);
            lt = fma4(f, X[par][u][1][L.quad], lt);
            svt = fma4(f, X[par][u][2][L.quad], svt);
            sst = fma4(f, X[par][u][3][L.quad], sst);
            ssvt = fma4(f, X[par][u][4][L.quad], ssvt);
            stvt = fma4(f, X[par][u][5][L.quad], stvt);
            if (u == w) fw = f;
        }
        const float4 inv = rcp4(lt);
        const float4 abar = woi * svt * inv;
        const float4 mm = sst * inv;
        const float4 gwoi = (ssvt - mm * svt + stvt) * inv;
        if (tid < QS && L.cok) st4(gwo + row * C + L.c0, gwoi);
        const float4 scale = fw * inv;
        T* ger = ge + row * NC;
        float4 gqa = f4(0.f);
#pragma unroll
        for (int t = 0; t < JPL; ++t) {
            const float4 ee = cvt_raw(re[t]);
            const float4 tee = cvt_raw(rte[t]);
            const float4 kk = kv[(0 * JPL + t) * kThreads + kl];
            const float4 vv = kv[(1 * JPL + t) * kThreads + kl];
            const float4 tkk = kv[(2 * JPL + t) * kThreads + kl];
            const float4 tvv = kv[(3 * JPL + t) * kThreads + kl];
            const float4 p = pe[t] * scale;
            // bwd2_slot() of attn_core.h with sbar centred (above); around the call the bf16 multi-slot instances allocate
            // differently
            const float4 a = woi * vv;
            const float4 g = gate(ee);
            const float4 g1 = dgate(ee);
            float4 ds = fma4(p, a - abar, ws ? cvt_raw(rws[t]) : f4(0.f));
            if (!L.jok[t]) ds = f4(0.f);
            const float4 pdot = p * (sd[t] - mm);
            const float4 sbar = p * fma4(sd[t] - mm, a - abar, woi * (tvv - gwoi));
            const float4 g1te = g1 * tee;
            gqa += sbar * kk * g + ds * fma4(tkk, g, kk * g1te);
            gkk[t] += sbar * aq * g + alpha * (ds * fma4(tqi, g, qi * g1te));
            gvv[t] = fma4(pdot, woi, gvv[t]);
            const float4 gev = sbar * aq * kk * g1 +
                               alpha * (ds * (g1 * fma4(tqi, kk, qi * tkk) + 2.f * (qi * kk * tee)));
            if (L.jok[t] && L.cok) st4_stream(ger + L.off[t], gev);
        }
        gqp = xor_sum4<QS>(gqa);
    }
    if (i1 > i0) {     // the last row's gq
        if (lane < QS) X[par][w][6][L.quad] = gqp;
        __syncthreads();
        if (tid < QS && L.cok) {
            float4 d = X[par][0][6][tid];
#pragma unroll
            for (int u = 1; u < 4; ++u) d += X[par][u][6][tid];
            st4(gq + (static_cast<size_t>(b) * N + i1 - 1) * C + L.c0, alpha * d);
        }
    }
    store_columns<T, JPL>(L, gkk, gvv, gk, gv, part, b, pl.group, G, B, NC);
}

// ------------------------------------------------------- column-sum merge ----
// (dk, dv)[x] = sum over the G row groups, ascending, of the float32 partials (part[0][g], part[1][g]); x runs over
// the float4s of one [B,N,C] tensor.
template <typename T>
__global__ __launch_bounds__(256) void attn_long_colsum_kernel(const float* __restrict__ part, T* __restrict__ a_out,
                                                               T* __restrict__ b_out, int64_t n4, int G) {
    const int64_t x = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (x >= n4) return;
    const size_t BNC = static_cast<size_t>(n4) * 4;
    float4 a = f4(0.f), c = f4(0.f);
    for (int g = 0; g < G; ++g) {
        a += ld4(part + g * BNC + 4 * x);
        c += ld4(part + (G + g) * BNC + 4 * x);
    }
    st4(a_out + 4 * x, a);
    st4(b_out + 4 * x, c);
}

// ---------------------------------------------------------------- dispatch ----
constexpr int kMaxN = 256;

// Slots per thread are what the registers allow without scratch (gfx950 resource report): the forward
// keeps up to 8 (32-channel slices, N <= 256); the backward up to 4 -- above 128 neighbours it takes 16-channel slices
// (64 phases); the second order up to 3 -- 16-channel slices up to 192 neighbours, 8-channel slices (128 phases) above.
enum LongOp { kOpFwd, kOpBwd, kOpBwd2 };
bool long_geometry(int N, int C, LongOp op, Geometry* g) {
    if (C < 8 || (C & 3) || N < 1 || N > kMaxN) return false;
    const int cq = C / 4;
    int lqs = (op != kOpBwd2 && cq >= 5) ? 3 : 2;
    const int max_jpl = op == kOpFwd ? 8 : (op == kOpBwd ? 4 : 3);
    while ((N + (kThreads >> lqs) - 1) / (kThreads >> lqs) > max_jpl) --lqs;
    const int need = (N + (kThreads >> lqs) - 1) / (kThreads >> lqs);
    g->lqs = lqs;
    g->slices = (cq + (1 << lqs) - 1) >> lqs;
    if (lqs == 3) g->jpl = need <= 2 ? 2 : (need <= 4 ? 4 : (need <= 6 ? 6 : 8));   // the instantiated slot counts
    else if (lqs == 1) g->jpl = 2;
    else g->jpl = need;     // 1..4
    return true;
}

int row_groups(int N, int rows) { return (N + rows - 1) / rows; }

size_t long_workspace_bytes(int B, int N, int C) {
    if (B < 1 || N < 1 || N > kMaxN || C < 8 || (C & 3)) return 0;
    const int G = row_groups(N, kBwdRows);
    return G > 1 ? static_cast<size_t>(2) * G * B * N * C * sizeof(float) : 0;
}

template <typename T>
int colsum(const void* part, void* a, void* b, int B, int N, int C, int G, hipStream_t stream) {
    const int64_t n4 = static_cast<int64_t>(B) * N * C / 4;
    hipLaunchKernelGGL((attn_long_colsum_kernel<T>), dim3(static_cast<unsigned>((n4 + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const float*>(part), static_cast<T*>(a), static_cast<T*>(b), n4, G);
    return 0;
}

// the instantiated (LQS, JPL)
using LongFwd = Shapes<Shape<3, 2>, Shape<3, 4>, Shape<3, 6>, Shape<3, 8>, Shape<2, 1>, Shape<2, 2>, Shape<2, 3>, Shape<2, 4>>;
using LongBwd = Shapes<Shape<3, 2>, Shape<3, 4>, Shape<2, 1>, Shape<2, 2>, Shape<2, 3>, Shape<2, 4>>;
using LongBwd2 = Shapes<Shape<2, 1>, Shape<2, 2>, Shape<2, 3>, Shape<1, 2>>;
constexpr const char* kNeed = " (need C%4==0, C>=8, 1<=N<=256)";

}  // namespace
}  // namespace dg

using namespace dg;

extern "C" size_t dg_attn_core_long_workspace_bytes(int B, int N, int C) { return long_workspace_bytes(B, N, C); }

extern "C" int dg_attn_core_long_fwd(const void* q_, const void* k_, const void* v_, const void* e_, void* s_, void* o_,
                                     int B, int N, int C, float alpha, int dtype, dg_stream_t stream_) {
    Geometry g;
    const bool ok = B >= 0 && long_geometry(N, C, kOpFwd, &g);
    if (int st = check_fwd("dg_attn_core_long_fwd", q_, k_, v_, e_, o_, dtype, {ok, B, N, C, kNeed})) return st;
    if (B == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int G = row_groups(N, kFwdRows);
    dim3 grid(static_cast<unsigned>((B + 7) / 8 * 8) * g.slices * G), block(kThreads);
    ProfScope prof(DG_K_ATTN_FWD, stream);
    const int reverse = take_direction(static_cast<int64_t>(B) * N * N);      // per-row results: any order
    return dispatch(LongFwd(), "dg_attn_core_long_fwd", dtype, g.lqs, g.jpl, [&](auto t, auto sh) {
        using T = decltype(t);
        using S = decltype(sh);
        hipLaunchKernelGGL((attn_long_fwd_kernel<T, S::LQS, S::JPL>), grid, block, 0, stream, static_cast<const T*>(q_),
                           static_cast<const T*>(k_), static_cast<const T*>(v_), static_cast<const T*>(e_),
                           static_cast<T*>(s_), static_cast<T*>(o_), N, C, alpha, g.slices, G, B, reverse);
        return 0;
    });
}

extern "C" int dg_attn_core_long_bwd(const void* q_, const void* k_, const void* v_, const void* e_, const void* ws_,
                                     const void* wo_, const void* add_e_, void* dq_, void* dk_, void* dv_, void* de_,
                                     void* workspace, size_t workspace_bytes, int B, int N, int C, float alpha,
                                     int dtype, dg_stream_t stream_) {
    Geometry g;
    const bool ok = B >= 0 && long_geometry(N, C, kOpBwd, &g);
    if (int st = check_bwd("dg_attn_core_long_bwd", q_, k_, v_, e_, wo_, dq_, dk_, dv_, de_, dtype, {ok, B, N, C, kNeed}))
        return st;
    const size_t need = long_workspace_bytes(B, N, C);
    if (need && (!workspace || workspace_bytes < need))
        return fail(DG_E_WORKSPACE, "dg_attn_core_long_bwd: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    if (B == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int G = row_groups(N, kBwdRows);
    dim3 grid(static_cast<unsigned>((B + 7) / 8 * 8) * g.slices * G), block(kThreads);
    ProfScope prof(DG_K_ATTN_BWD, stream);
    const int reverse = take_direction(static_cast<int64_t>(B) * N * N);      // per-group results: any order
    float* part = static_cast<float*>(workspace);
    return dispatch(LongBwd(), "dg_attn_core_long_bwd", dtype, g.lqs, g.jpl, [&](auto t, auto sh) {
        using T = decltype(t);
        constexpr int LQS = decltype(sh)::LQS, JPL = decltype(sh)::JPL;
        constexpr int lds = (2 * JPL * kThreads + 2 * 4 * 4 * (1 << LQS)) * 16;
        auto launch = [&](auto adde) {
            constexpr bool ADDE = decltype(adde)::value;
            DG_OPT_IN_LDS((&attn_long_bwd_kernel<T, LQS, JPL, ADDE>), lds);
            hipLaunchKernelGGL((attn_long_bwd_kernel<T, LQS, JPL, ADDE>), grid, block, lds, stream,
                               static_cast<const T*>(q_), static_cast<const T*>(k_), static_cast<const T*>(v_),
                               static_cast<const T*>(e_), static_cast<const T*>(ws_), static_cast<const T*>(wo_),
                               static_cast<const T*>(add_e_), static_cast<T*>(dq_), static_cast<T*>(dk_),
                               static_cast<T*>(dv_), static_cast<T*>(de_), part, N, C, alpha, g.slices, G, B, reverse);
            return G > 1 ? colsum<T>(part, dk_, dv_, B, N, C, G, stream) : 0;
        };
        return add_e_ ? launch(std::true_type()) : launch(std::false_type());
    });
}

extern "C" int dg_attn_core_long_bwd2(const void* q_, const void* k_, const void* v_, const void* e_, const void* ws_,
                                      const void* wo_, const void* tq_, const void* tk_, const void* tv_, const void* te_,
                                      void* gq_, void* gk_, void* gv_, void* ge_, void* gws_, void* gwo_, void* workspace,
                                      size_t workspace_bytes, int B, int N, int C, float alpha, int dtype,
                                      dg_stream_t stream_) {
    Geometry g;
    const bool ok = B >= 0 && long_geometry(N, C, kOpBwd2, &g);
    if (int st = check_bwd2("dg_attn_core_long_bwd2", q_, k_, v_, e_, wo_, tq_, tk_, tv_, te_, gq_, gk_, gv_, ge_, gwo_, dtype,
                            {ok, B, N, C, kNeed}))
        return st;
    const size_t need = long_workspace_bytes(B, N, C);
    if (need && (!workspace || workspace_bytes < need))
        return fail(DG_E_WORKSPACE, "dg_attn_core_long_bwd2: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    if (B == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int G = row_groups(N, kBwdRows);
    dim3 grid(static_cast<unsigned>((B + 7) / 8 * 8) * g.slices * G), block(kThreads);
    ProfScope prof(DG_K_ATTN_BWD2, stream);
    const int reverse = take_direction(static_cast<int64_t>(B) * N * N);      // per-group results: any order
    float* part = static_cast<float*>(workspace);
    return dispatch(LongBwd2(), "dg_attn_core_long_bwd2", dtype, g.lqs, g.jpl, [&](auto t, auto sh) {
        using T = decltype(t);
        constexpr int LQS = decltype(sh)::LQS, JPL = decltype(sh)::JPL;
        constexpr int lds = (4 * JPL * kThreads + 2 * 4 * 7 * (1 << LQS)) * 16;
        DG_OPT_IN_LDS((&attn_long_bwd2_kernel<T, LQS, JPL>), lds);
        hipLaunchKernelGGL((attn_long_bwd2_kernel<T, LQS, JPL>), grid, block, lds, stream,
                           static_cast<const T*>(q_), static_cast<const T*>(k_), static_cast<const T*>(v_),
                           static_cast<const T*>(e_), static_cast<const T*>(ws_), static_cast<const T*>(wo_),
                           static_cast<const T*>(tq_), static_cast<const T*>(tk_), static_cast<const T*>(tv_),
                           static_cast<const T*>(te_), static_cast<T*>(gq_), static_cast<T*>(gk_),
                           static_cast<T*>(gv_), static_cast<T*>(ge_), static_cast<T*>(gws_), static_cast<T*>(gwo_),
                           part, N, C, alpha, g.slices, G, B, reverse);
        return G > 1 ? colsum<T>(part, gk_, gv_, B, N, C, G, stream) : 0;
    });
}
