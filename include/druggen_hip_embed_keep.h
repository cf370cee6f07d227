/* druggen_hip_embed_keep.h -- add-on to druggen_hip.h: the general edge embedding (csrc/embed_sym_keep.hip) with the
 * forward's signs kept for the backward kernels.  Conventions (pointers, dtype, status codes, stream) as in druggen_hip.h;
 * the ctypes table of these entries is druggen_amd/_lib.py::EMBED_KEEP_SIGNATURES.                                       */
#ifndef DRUGGEN_HIP_EMBED_KEEP_H
#define DRUGGEN_HIP_EMBED_KEEP_H

#include "druggen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The same three entries with the forward's signs KEPT instead of recomputed, for the piecewise-linear activations (act =
 * relu, leaky; others: DG_E_ARG).  Same library and DG_VERSION as druggen_hip.h, whose entries are unchanged.
 * `signs`: dg_embed_sym_sign_words(B, N) uint32 words, six per edge row r = (b N + i) N + j at signs[6 r ..]:
 *   words 0..3: bit (c & 31) of word (c >> 5) is set iff the layer-2 pre-activation (bias included) of channel c is > 0,
 *   words 4..5: bit (u & 31) of word 4 + (u >> 5) is set iff the layer-1 pre-activation of hidden unit u is > 0.
 * _fwd_keep writes the output of dg_embed_sym_fwd (bit for bit) and every word of `signs`.  _bwd_keep and _bwd2_keep
 * read the signs in place of both recomputed layers and return, bit for bit, what _bwd / _bwd2 return -- for the outputs
 * that are wanted: da may be NULL; dw1, db1, dw2, db2 are all non-NULL or all NULL (a mixture: DG_E_ARG; nothing wanted:
 * 0 without a launch); gw1, gw2 are both non-NULL or both NULL.  Without weight gradients _bwd_keep reads neither `a` nor
 * the workspace, and _bwd2_keep reads neither `a` nor `g`; the pointers are still checked.                           */
size_t dg_embed_sym_sign_words(int B, int N);
int dg_embed_sym_fwd_keep(const float* a, const float* w1, const float* b1, const float* w2_packed, const float* b2,
                          void* out, uint32_t* signs, int B, int N, int E, int H, int C, int act, int dtype,
                          dg_stream_t stream);
int dg_embed_sym_bwd_keep(const float* a, const float* w1, const float* b1, const float* w2_packed,
                          const float* w2_dgrad_packed, const float* b2, const void* g, const uint32_t* signs,
                          float* da, float* dw1, float* db1, float* dw2, float* db2,
                          void* workspace, size_t workspace_bytes,
                          int B, int N, int E, int H, int C, int act, int dtype, dg_stream_t stream);
int dg_embed_sym_bwd2_keep(const float* a, const float* w1, const float* b1, const float* w2_packed,
                           const float* w2_dgrad_packed, const float* b2, const void* g, const float* t,
                           const uint32_t* signs, void* gg, float* gw1, float* gw2, void* workspace,
                           size_t workspace_bytes, int B, int N, int E, int H, int C, int act, int dtype,
                           dg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DRUGGEN_HIP_EMBED_KEEP_H */
