// Host entry points of the training attention kernels.
//
// Included by the four attention .hip files that define them and by
// bindings.cpp that calls them, so the compiler checks every definition
// and every call against one declaration (with C linkage a hand-copied
// prototype that drifts still links).
//
// Layouts: Q, O, dO, dQ [B,S,Hq,ATT_D]; K, V, dK, dV [B,S,Hkv,ATT_D];
// lse, Dvec [B,Hq,S] fp32.  All bf16 tensors are contiguous; S % 64 == 0
// and Hq % Hkv == 0 (checked in bindings.cpp).
#pragma once

#include <hip/hip_runtime.h>

#define ATT_D 128  // head dim every attention kernel is written for

extern "C" {
// Dispatchers: pick the v3 kernels or the 64-tile kernels from S.
void attn_fwd_launch(const void* Q, const void* K, const void* V, void* O,
                     float* lse, int B, int S, int Hq, int Hkv, float scale,
                     bool causal, hipStream_t stream);
void attn_bwd_launch(const void* Q, const void* K, const void* V,
                     const void* O, const void* dO, const float* lse,
                     float* Dvec, void* dQ, void* dK, void* dV, int B, int S,
                     int Hq, int Hkv, float scale, bool causal,
                     int dkv_variant, int dq_variant, hipStream_t stream);

// v3 kernels: forward needs S % 256 == 0, backward S % 128 == 0.
void attn_fwd_v3_launch(const void* Q, const void* K, const void* V, void* O,
                        float* lse, int B, int S, int Hq, int Hkv,
                        float scale, bool causal, hipStream_t stream);
void attn_bwd_v3_launch(const void* Q, const void* K, const void* V,
                        const void* dO, const float* lse, const float* Dvec,
                        void* dQ, void* dK, void* dV, int B, int S, int Hq,
                        int Hkv, float scale, bool causal, int dkv_variant,
                        int dq_variant, hipStream_t stream);
}
