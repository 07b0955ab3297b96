// Host entry point of the multi-token verify attention
// (attention_verify.hip), declared once for the definition and for
// bindings.cpp.  The split rule is the grouped decode kernel's
// (gqa_split_rows, attn_decode_gqa.h).
#pragma once

#include <hip/hip_runtime.h>

#include "attn_decode_gqa.h"

// Columns (token, q head of the group) one block takes: two 16-column MFMA
// blocks.  T * (Hq / Hkv) must not exceed it.
#define VERIFY_MAX_COLS 32

extern "C" {
// Ow fp32 [n, T, Hq, splits, 128] and MLw fp32 [n, T, Hq, splits, 2] are
// only touched when splits > 1.  split_rows is the resolved rows per split.
void attn_verify_launch(const void* Q, const void* Kc, const void* Vc,
                        void* O, void* Ow, void* MLw, const int* slot_ids,
                        const int* q_start, int n, int T, int S_max, int Hq,
                        int Hkv, int split_rows, int splits, float scale,
                        hipStream_t stream);
}
