// Host entry point of the serving append-attention kernel
// (attention_append.hip), declared once for the definition and for
// bindings.cpp, like attn_launch.h does for the training kernels.
//
// Layouts: Q, O [n,Sq,Hq,ATT_D]; Kc, Vc [slots,S_max,Hkv,ATT_D], all bf16
// and contiguous; slot_ids, q_start, q_lens int32 [n] on the device.
// Sq % 64 == 0, Hq % Hkv == 0, n*Hq <= 65535 (checked in bindings.cpp).
#pragma once

#include "attn_launch.h"

extern "C" {
void attn_append_launch(const void* Q, const void* Kc, const void* Vc,
                        void* O, const int* slot_ids, const int* q_start,
                        const int* q_lens, int n, int Sq, int Hq, int Hkv,
                        int slots, int S_max, float scale,
                        hipStream_t stream);
}
