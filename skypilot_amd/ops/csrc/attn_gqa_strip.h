// Device pieces that the grouped split-KV decode kernel
// (attention_decode_gqa.hip) and the multi-token verify kernel
// (attention_verify.hip) share: the 32-row strip of the bf16 cache as it is
// loaded, and the staging of its V rows into the wave's LDS tile.
#pragma once

#include "common.h"

#define GQA_D 128
#define GQA_STRIP_ROWS 32
// One wave's LDS: the [128 d][32 k-slot] bf16 V tile (8 KB) in the row
// loop, then its O^T partial as [16 q][132] fp32 (padded rows).
#define GQA_O_STRIDE 132
#define GQA_WAVE_FLOATS (16 * GQA_O_STRIDE)

__device__ __forceinline__ float gqa_exp2(float x) {
  return __builtin_amdgcn_exp2f(x);
}

// bf16 cache: K fragments and V row chunks of one strip, as loaded.
struct GqaStripBf16 {
  s16x8 k[8];  // [4mb + ks]: row 16mb + (l&15), d = 32ks + 8(l>>4)
  s16x8 v[8];  // [4mb + r]:  row 16mb + 4(l>>4) + r, d = 8(l&15)
  __device__ __forceinline__ void load(const unsigned short* Kb,
                                       const unsigned short* Vb,
                                       long long rs, int base, int end,
                                       int lane) {
    const int kb = lane >> 4, lr = lane & 15;
    const bool full = base + GQA_STRIP_ROWS <= end;  // wave-uniform
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int krow = base + 16 * mb + lr;
      const unsigned short* kr =
          Kb + (long long)(full ? krow : min(krow, end - 1)) * rs + 8 * kb;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        k[4 * mb + ks] = *(const s16x8*)(kr + 32 * ks);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int vrow = base + 16 * mb + 4 * kb + r;
        const s16x8 vv = *(const s16x8*)(
            Vb + (long long)(full ? vrow : min(vrow, end - 1)) * rs + 8 * lr);
        v[4 * mb + r] =
            (full || vrow < end) ? vv : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
  }
  __device__ __forceinline__ s16x8 kfrag(int i) const { return k[i]; }
  __device__ __forceinline__ s16x8 vrow(int i) const { return v[i]; }
};

union gqa_cast {
  s16x8 s;
  i32x4 w;
};

// V of one strip into the wave's [d][k-slot] tile `vt`: four rows of one d
// -> 8 bytes at k-slots 8kb + 4mb .. +3.  (kb, lr) = (lane >> 4, lane & 15).
template <class Strip>
__device__ __forceinline__ void gqa_stage_v(const Strip& st, char* vt,
                                            int kb, int lr) {
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    gqa_cast r0, r1, r2, r3;
    r0.s = st.vrow(4 * mb + 0);
    r1.s = st.vrow(4 * mb + 1);
    r2.s = st.vrow(4 * mb + 2);
    r3.s = st.vrow(4 * mb + 3);
#pragma unroll
    for (int wi = 0; wi < 4; ++wi) {
      const unsigned a0 = (unsigned)r0.w[wi], a1 = (unsigned)r1.w[wi];
      const unsigned a2 = (unsigned)r2.w[wi], a3 = (unsigned)r3.w[wi];
      const i32x2 lo = {(int)((a0 & 0xffffu) | (a1 << 16)),
                        (int)((a2 & 0xffffu) | (a3 << 16))};
      const i32x2 hi = {(int)((a0 >> 16) | (a1 & 0xffff0000u)),
                        (int)((a2 >> 16) | (a3 & 0xffff0000u))};
      // d = 8 lr + e lives in tile row e * 16 + lr
      *(i32x2*)(vt + ((2 * wi) * 16 + lr) * 64 + 16 * kb + 8 * mb) = lo;
      *(i32x2*)(vt + ((2 * wi + 1) * 16 + lr) * 64 + 16 * kb + 8 * mb) = hi;
    }
  }
}

// The A fragment of O^T += V^T P^T for d rows 16ct + (l&15), read back
// from the tile gqa_stage_v wrote.
__device__ __forceinline__ s16x8 gqa_v_frag(const char* vt, int ct, int kb,
                                            int lr) {
  return *(const s16x8*)(
      vt + ((lr & 7) * 16 + 2 * ct + (lr >> 3)) * 64 + 16 * kb);
}
