// Host entry points of the FP8 KV-cache kernels (kv_write_fp8.hip,
// attention_decode_fp8.hip, attention_append.hip), declared once for the
// definitions and for bindings.cpp.
//
// Code tensors Kc, Vc are uint8 [slots,S_max,Hkv,128]; exponent tensors
// Ke, Ve are uint8 [slots,S_max,Hkv]; everything is contiguous and the
// index tensors are int32 on the device (checked in bindings.cpp).
#pragma once

#include <hip/hip_runtime.h>

extern "C" {
void kv_write_fp8_launch(const void* k, const void* v, void* Kc, void* Vc,
                         void* Ke, void* Ve, const int* slot_ids,
                         const int* starts, const int* lens, int n, int S,
                         int Hkv, int slots, int S_max, hipStream_t stream);
void attn_decode_qkv_fp8_launch(const void* qkv, void* Kc, void* Vc,
                                void* Ke, void* Ve, void* O,
                                const void* cos_tab, const void* sin_tab,
                                const int* positions, const int* kv_lens,
                                const int* slot_ids, int B, int S_max,
                                int Hq, int Hkv, float scale,
                                hipStream_t stream);
void attn_append_fp8_launch(const void* Q, const void* Kc, const void* Vc,
                            const void* Ke, const void* Ve, void* O,
                            const int* slot_ids, const int* q_start,
                            const int* q_lens, int n, int Sq, int Hq,
                            int Hkv, int slots, int S_max, float scale,
                            hipStream_t stream);
}
