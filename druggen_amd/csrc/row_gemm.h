// Host entry points of the float32 row GEMM (row_gemm.hip), called from the dtype dispatch of the public C ABI
// (gemm_bf16.hip).  The default arguments live here only.
#pragma once

#include "common.h"

namespace dg {

size_t row_gemm_f32_packed_floats(int n_out, int k_contract);
int row_gemm_f32_pack(const float* w, float* packed, int rows, int cols, int mode, dg_stream_t stream,
                      const float* w1 = nullptr, const float* w2 = nullptr);
int row_gemm_f32_lin3(const float* a, const float* packed, float* y0, float* y1, float* y2, int64_t R, const float* b0,
                      const float* b1, const float* b2, dg_stream_t stream);
int row_gemm_f32_sum3(const float* a0, const float* a1, const float* a2, const float* packed, float* y, int64_t R,
                      const float* residual, dg_stream_t stream);
size_t row_gemm_f32_mask_words(int64_t R, int K, int N);
int row_gemm_f32_pack_batch(const void* table, int n, int max_rows_cols, dg_stream_t stream);
size_t row_gemm_f32_ln_bwd_workspace_bytes();
int row_gemm_f32_ln_bwd(const float* a, const float* packed, float* dz, int64_t R, int K, const float* residual,
                        const float* pre, const float* mean, const float* rstd, const float* gamma, float* dgamma,
                        float* dbeta, void* workspace, size_t workspace_bytes, dg_stream_t stream);
int row_gemm_f32_ln_in(const float* dy, const float* pre, const float* mean, const float* rstd, const float* gamma,
                       const float* packed, float* dz, float* y, float* dgamma, float* dbeta, void* workspace,
                       size_t workspace_bytes, int64_t R, dg_stream_t stream);
int row_gemm_f32(const float* a, const float* packed, float* y, int64_t R, int K, int N, const float* bias, int relu,
                 unsigned* relu_bits_out, const unsigned* mask_bits, const float* residual, const float* gamma,
                 const float* beta, float* mean, float* rstd, float* pre_ln, float eps, dg_stream_t stream,
                 const float* ascale = nullptr, float* yscale = nullptr, int afmt = 0, int yfmt = 0, const void* alo = nullptr,
                 void* ylo = nullptr);

}  // namespace dg
