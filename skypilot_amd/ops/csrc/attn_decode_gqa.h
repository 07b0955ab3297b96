// Host entry points and the split rule of the grouped split-KV decode
// attention (attention_decode_gqa.hip), declared once for the definitions
// and for bindings.cpp.
#pragma once

#include <hip/hip_runtime.h>

// Cache rows per split when the caller passes split_rows = -1.  One
// constant, not a per-batch table: a sequence's output bits must not depend
// on the batch it rides in (docs/KERNELS.md, "Grouped split-KV decode").
#define kDecodeSplitRows 512
#define GQA_MAX_GROUP 16
#define GQA_MAX_SPLITS 64

// Rows per split for a cache of S_max rows: a function of S_max and the
// requested value only; doubled until at most GQA_MAX_SPLITS splits remain.
static inline int gqa_split_rows(long long S_max, int split_rows) {
  long long R = split_rows < 0 ? kDecodeSplitRows : split_rows;
  while ((S_max + R - 1) / R > GQA_MAX_SPLITS) R *= 2;
  return (int)R;
}

extern "C" {
// Ow fp32 [n, Hq, splits, 128] and MLw fp32 [n, Hq, splits, 2] are only
// touched when splits > 1.
void attn_decode_gqa_launch(const void* qkv, void* Kc, void* Vc, void* O,
                            void* Ow, void* MLw, const void* cos_tab,
                            const void* sin_tab, const int* positions,
                            const int* kv_lens, const int* slot_ids, int n,
                            int S_max, int Hq, int Hkv, int split_rows,
                            int splits, float scale, hipStream_t stream);
void attn_decode_gqa_fp8_launch(const void* qkv, void* Kc, void* Vc,
                                void* Ke, void* Ve, void* O, void* Ow,
                                void* MLw, const void* cos_tab,
                                const void* sin_tab, const int* positions,
                                const int* kv_lens, const int* slot_ids,
                                int n, int S_max, int Hq, int Hkv,
                                int split_rows, int splits, float scale,
                                hipStream_t stream);
}
