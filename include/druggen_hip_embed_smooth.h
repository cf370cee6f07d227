/* druggen_hip_embed_smooth.h -- add-on to druggen_hip.h: the second order of the edge embedding for the smooth
 * activations (csrc/embed_sym_smooth.hip).  Conventions (pointers, dtype, status codes, stream) as in druggen_hip.h; the
 * ctypes table of this entry is druggen_amd/_lib.py::EMBED_SMOOTH_SIGNATURES.                                            */
#ifndef DRUGGEN_HIP_EMBED_SMOOTH_H
#define DRUGGEN_HIP_EMBED_SMOOTH_H

#include "druggen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Backward of dg_embed_sym_bwd for the gradient penalty, act = sigmoid (2) or tanh (3).  With act'' != 0 the adjoint t
 * [B,N,N,E] of da reaches every operand of the forward, not only g, w1 and w2 as in dg_embed_sym_bwd2.  Per edge row, gs
 * = the symmetrised upstream gradient, u1 / u2 = the pre-activations of the two layers, h1 = act(u1):
 *   p2 = gs act'(u2), dh1 = W2^T p2, p1 = dh1 act'(u1)                          (the first backward, recomputed)
 *   s1 = W1 t, q = s1 act'(u1), s2 = W2 q, x = s2 act'(u2)                      gg = (x_ij + x_ji) / 2
 *   r2 = gs act''(u2) s2,  r1 = act''(u1) s1 dh1 + act'(u1) (W2^T r2)
 *   gw2 = sum p2 q^T + r2 h1^T, gb2 = sum r2, gw1 = sum p1 t^T + r1 a^T, gb1 = sum r1, ga = W1^T r1 (per row)
 * Operands as dg_embed_sym_bwd2.  Outputs: gg [B,N,N,C] (dtype) = adjoint of g; ga [B,N,N,E] = adjoint of a (fp32, may be
 * NULL); gw1 [H,E], gb1 [H], gw2 [C,H], gb2 [C] (fp32): all four non-NULL or all four NULL (a mixture: DG_E_ARG).  NULL
 * skips the stages of that output, and for the parameters the reduction and the workspace too; what remains is bit for
 * bit what the full call returns.  Workspace: dg_embed_sym_workspace_bytes(B, N) (too small: DG_E_WORKSPACE).  act = relu,
 * leaky: DG_E_ARG (dg_embed_sym_bwd2 is their entry).  No atomics; the grid is fixed by the shape: bit-reproducible.   */
int dg_embed_sym_bwd2_smooth(const float* a, const float* w1, const float* b1, const float* w2_packed,
                             const float* w2_dgrad_packed, const float* b2, const void* g, const float* t,
                             void* gg, float* ga, float* gw1, float* gb1, float* gw2, float* gb2,
                             void* workspace, size_t workspace_bytes,
                             int B, int N, int E, int H, int C, int act, int dtype, dg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DRUGGEN_HIP_EMBED_SMOOTH_H */
