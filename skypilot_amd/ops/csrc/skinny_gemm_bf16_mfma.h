// Launcher interface of the bf16-weight MFMA decode GEMM
// (skinny_gemm_bf16_mfma.hip).
#pragma once

#include <hip/hip_runtime.h>

extern "C" {
// Resolves row_tiles / k_splits: a 0 becomes the launcher's own choice, a
// function of (I, O) alone; other values are kept.
void skinny_gemm_bf16_mfma_plan(int I, int O, int* row_tiles, int* k_splits);
// Y[n, O] bf16 = X[n, I] @ W[O, I]^T.  row_tiles in {1, 2, 4}, k_splits in
// {1, 2, 4, 8}, both resolved; partials is fp32 [k_splits, n, O] and is
// read and written only when k_splits > 1.
void skinny_gemm_bf16_mfma_launch(const void* W, const void* X, void* Y,
                                  float* partials, int n, int I, int O,
                                  int row_tiles, int k_splits,
                                  hipStream_t stream);
}
