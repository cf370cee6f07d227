/* druggen_hip_node_wide.h -- add-on to druggen_hip.h: the node-side layers of a model whose node matrices are wider than 16
 * columns (the reference's --features: m_dim = atom types + 54 descriptor columns; csrc/node_wide.hip).
 * Conventions (pointers, status codes, stream) as in druggen_hip.h; the ctypes table of these entries is
 * druggen_amd/_lib.py::NODE_WIDE_SIGNATURES.  Everything is float32 fmaf arithmetic without atomics: results are
 * bit-identical from run to run.                                                                                          */
#ifndef DRUGGEN_HIP_NODE_WIDE_H
#define DRUGGEN_HIP_NODE_WIDE_H

#include "druggen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Node embedding Linear(E, 64) - act - Linear(64, 128) - act for 1 <= E <= 255 (the resident store's limit on m_dim).
 * dg_embed_node_wide_chain has the contract of dg_embed_node_chain (forward with m1 = m2 = NULL for act 0..3; m1 / m2 given: the
 * masked second-order form, act 0 / 1 only, act 2 / 3: DG_E_ARG), dg_embed_node_wide_bwd that of dg_embed_node_bwd (dz may be
 * NULL).  Every sum runs bias first, one accumulator per output, inputs in ascending index: for E <= 16 the results equal the
 * narrow entries' bit for bit.  E outside 1..255: DG_E_SHAPE; R == 0 returns 0 without a launch.                              */
int dg_embed_node_wide_chain(const float* in, const float* m1, const float* m2, const float* w1, const float* b1,
                             const float* w2, const float* b2, float* o1, float* o2, int64_t R, int E, int act,
                             dg_stream_t stream);
int dg_embed_node_wide_bwd(const float* g, const float* a1, const float* a2, const float* w1, const float* w2, float* g2,
                           float* g1, float* dz, int64_t R, int E, int act, dg_stream_t stream);

/* Weight gradient of the first Linear: dw1 [64,E] = g1^T z, db1 [64] = column sums of g1 (db1 may be NULL: the second-order
 * twin g1^T t has no bias) from g1 [R,64] and z [R,E].  The rows are split over workgroups in a way that depends on R only,
 * the partial sums go to `workspace` (dg_embed_node_wide_wgrad_workspace_bytes(R, E); 0 for an unsupported shape; a shorter
 * one: DG_E_WORKSPACE) and are added in a fixed order.  R >= 1, 1 <= E <= 255: others DG_E_SHAPE.                            */
size_t dg_embed_node_wide_wgrad_workspace_bytes(int64_t R, int E);
int dg_embed_node_wide_wgrad(const float* g1, const float* z, float* dw1, float* db1, void* workspace, size_t workspace_bytes,
                             int64_t R, int E, dg_stream_t stream);

/* Wide readout: nn.Linear(128 -> N), 17 <= N <= 255 (readout_n of a --features Generator, reference models.py:100-101), with
 * the semantics of dg_skinny_linear_fwd / _dgrad / _wgrad: x [R,128] in the activation dtype (`dtype`: DG_DTYPE_F32 or
 * DG_DTYPE_BF16), w [N,128], b [N] or NULL, y [R,N] float32; _dgrad: dx [R,128] (activation dtype) = dy [R,N] (float32) . w;
 * _wgrad: dw [N,128] = dy^T x, db [N] (nullable) = column sums of dy, partial sums in `workspace`
 * (dg_wide_linear_wgrad_workspace_bytes(R, N, K)) as for dg_embed_node_wide_wgrad.  K != 128 or N outside 17..255: DG_E_SHAPE;
 * R == 0 returns 0 without a launch (_fwd, _dgrad; _wgrad needs R >= 1).                                                      */
int dg_wide_linear_fwd(const void* x, const float* w, const float* b, float* y, int64_t R, int N, int K, int dtype,
                       dg_stream_t stream);
int dg_wide_linear_dgrad(const float* dy, const float* w, void* dx, int64_t R, int N, int K, int dtype, dg_stream_t stream);
size_t dg_wide_linear_wgrad_workspace_bytes(int64_t R, int N, int K);
int dg_wide_linear_wgrad(const float* dy, const void* x, float* dw, float* db, void* workspace, size_t workspace_bytes,
                         int64_t R, int N, int K, int dtype, dg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DRUGGEN_HIP_NODE_WIDE_H */
