/* druggen_hip_row_gemm_any.h -- add-on to druggen_hip.h: the float32 row GEMM of nn.Linear layers whose widths are not the
 * three dg_row_gemm owns (the reference's --dim / --mlp_ratio; csrc/row_gemm_any.hip).  Conventions (pointers,
 * status codes, stream) as in druggen_hip.h; the ctypes table of these entries is druggen_amd/_lib.py::ROW_GEMM_ANY_SIGNATURES.
 * Same arithmetic class as dg_row_gemm for float32 rows: fp16 hi + lo planes under a power-of-two scale per activation row and
 * per output channel, three MFMA products, float32 accumulation in a fixed order over K that does not depend on R -- results
 * are bit-identical from run to run, and a row's result does not depend on the rows around it.                            */
#ifndef DRUGGEN_HIP_ROW_GEMM_ANY_H
#define DRUGGEN_HIP_ROW_GEMM_ANY_H

#include "druggen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the packed copy of a weight with n_out output channels and a contraction of k: both multiples of 32 in
 * [32, 1024]; 0 for any other shape.                                                                                      */
size_t dg_row_gemm_any_packed_bytes(int n_out, int k);

/* Pack the float32 nn.Linear weight w [rows, cols] into MFMA fragment order (hi / lo planes, inverse channel scales).
 * mode 0: the forward operand (y = a w^T: n_out = rows, k = cols); mode 1: the input-gradient operand (y = a w: n_out = cols,
 * k = rows).  Null w / packed or another mode: DG_E_ARG; rows / cols not a multiple of 32 in [32, 1024]: DG_E_SHAPE.       */
int dg_row_gemm_any_pack(const float* w, void* packed, int rows, int cols, int mode, dg_stream_t stream);

/* y [R,N] = a [R,K] . B (+ bias [N]; bias may be NULL) with B the operand packed for (n_out = N, k = K).  Null a / packed / y:
 * DG_E_ARG; R < 0, or K / N not a multiple of 32 in [32, 1024]: DG_E_SHAPE; R == 0 returns 0 without a launch.  The three
 * shapes of dg_row_gemm are served too (with a pack made by dg_row_gemm_any_pack).                                         */
int dg_row_gemm_any(const float* a, const void* packed, const float* bias, float* y, int64_t R, int K, int N,
                    dg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DRUGGEN_HIP_ROW_GEMM_ANY_H */
