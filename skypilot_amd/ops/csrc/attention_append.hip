// Append attention (chunked prefill) for the serving engine: Sq new
// tokens per sequence attend the rows already in the slot KV cache plus
// their own, which the caller has written into the cache before the
// launch.  Causal, GQA, D=128, bf16, CDNA4/gfx950.
//
// Structure is attn_fwd_swapped_kernel's (attention_fwd.hip): 64 q rows
// per 256-thread block, kv tiles of 64, S^T = K Q^T so the online
// softmax is per lane, P^T shuffled into B-fragments, swz/swzT LDS
// tiles, K/V global loads issued one tile ahead.  What differs:
//
//  * K/V come from the cache slot of the sequence, and the causal
//    diagonal sits at q_start + i, not i.  slot, q_start and q_len are
//    read from device tensors (no host sync) and are wave-uniform.
//  * Only rows [0, kv_len) of the slot, kv_len = min(q_start + q_len,
//    S_max), are this sequence's.  Everything past them is stale or
//    uninitialised memory, possibly NaN/Inf, and S_max is not a multiple
//    of 64, so a 64-row tile can run past kv_len and, in the last slot,
//    past the allocation.  A tile that does not lie wholly below kv_len
//    clamps every global row index to kv_len - 1 (the prologue and the
//    kt+1 prefetch alike, both through append_load_tile); V rows at or
//    past kv_len are staged as zeros because 0 * NaN in the PV MFMA is
//    NaN; K there is the clamped (valid) row and its score is masked.
//    Tiles wholly below kv_len take the parent's unclamped loads
//    (measured: 1.056x -> 1.010x the parent's time on identical work).
//  * Chunk rows at or past q_len are padding.  A q tile made of padding
//    only stores zeros and returns; padding rows inside a partly valid
//    tile get the attention of their position, which is finite.
//  * No lse output (inference only).
//
// The kernel body (attn_append_body.h) is included once per K/V source:
// the bf16 cache described above, and AppendTileFp8, which reads the FP8
// KV cache (kv_fp8.h): 8-byte chunks of e4m3fn codes plus the row's
// exponent byte,
// with the same clamp to kv_len - 1 for the codes and for the exponent and
// the same zero V rows; staging converts code * 2^n to bf16, which is
// exact, before the swz/swzT LDS writes.  From the first barrier on the
// two instantiations run the same code on the same LDS contents, so
// attn_append_fp8 equals attn_append on the dequantised cache bit for bit.
#include "attn_append.h"
#include "common.h"
#include "kv_fp8.h"

#define BM 64  // q rows per block
#define BN 64  // kv rows per tile

// One thread's share of a 64-row K/V tile: chunk (tid&7)|((i&1)<<3) of
// row (tid>>3)|((i>>1)<<5), i = 0..3 (the parent kernel's map).
__device__ __forceinline__ void append_load_tile(
    const unsigned short* __restrict__ Kb,
    const unsigned short* __restrict__ Vb, long long kv_rowstride,
    int kvbase, int kv_len, int tid, s16x8* kpre, s16x8* vpre) {
  if (kvbase + BN <= kv_len) {
    // Whole tile valid (block-uniform): the parent's loads, per-thread
    // offsets loop-invariant, no clamp and no select.
    const long long base = (long long)kvbase * kv_rowstride;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int s_ch = (tid & 7) | ((i & 1) << 3);
      const int s_row = (tid >> 3) | ((i >> 1) << 5);
      const long long r = base + (long long)s_row * kv_rowstride + s_ch * 8;
      kpre[i] = *(const s16x8*)(Kb + r);
      vpre[i] = *(const s16x8*)(Vb + r);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s_ch = (tid & 7) | ((i & 1) << 3);
    const int s_row = (tid >> 3) | ((i >> 1) << 5);
    const int row = kvbase + s_row;
    const int row_c = min(row, kv_len - 1);  // never past the valid rows
    const long long r = (long long)row_c * kv_rowstride + s_ch * 8;
    kpre[i] = *(const s16x8*)(Kb + r);
    const s16x8 vv = *(const s16x8*)(Vb + r);
    vpre[i] = (row < kv_len) ? vv : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }
}

// The FP8 K/V source of the kernel body: load() fetches one thread's share
// of a tile into registers (issued one tile ahead), k(i) / v(i) hand the
// staging loop chunk i as 8 bf16.  Same chunk/row map; a chunk of 8 elements is 8 bytes of codes, and the
// thread's four chunks lie in two rows ((tid>>3) and (tid>>3)+32), so it
// carries two exponents per tensor.
struct AppendTileFp8 {
  const unsigned char* Kb;
  const unsigned char* Vb;
  const unsigned char* Keb;
  const unsigned char* Veb;
  long long kv_rowstride;
  int Hkv;
  i32x2 kpre[4], vpre[4];
  unsigned ke[2], ve[2];  // exponent bytes of rows (tid>>3), (tid>>3)+32
  __device__ __forceinline__ AppendTileFp8(const unsigned char* Kc,
                                           const unsigned char* Vc,
                                           const unsigned char* Ke,
                                           const unsigned char* Ve,
                                           long long row0,
                                           long long rowstride, int Hkv_)
      : Kb(Kc + row0 * ATT_D),
        Vb(Vc + row0 * ATT_D),
        Keb(Ke + row0),
        Veb(Ve + row0),
        kv_rowstride(rowstride), Hkv(Hkv_) {}
  __device__ __forceinline__ void load(int kvbase, int kv_len, int tid) {
    if (kvbase + BN <= kv_len) {
      // Whole tile valid (block-uniform): plain loads, no clamp and no
      // select, so nothing consumes a register before the staging loop
      // and the loads stay in flight under the MFMAs.
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const long long row = kvbase + ((tid >> 3) | (h << 5));
        ke[h] = Keb[row * Hkv];
        ve[h] = Veb[row * Hkv];
#pragma unroll
        for (int lo = 0; lo < 2; ++lo) {
          const long long r =
              row * kv_rowstride + ((tid & 7) | (lo << 3)) * 8;
          kpre[2 * h + lo] = *(const i32x2*)(Kb + r);
          vpre[2 * h + lo] = *(const i32x2*)(Vb + r);
        }
      }
      return;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = kvbase + ((tid >> 3) | (h << 5));
      // never past the valid rows, codes and exponent alike
      const long long row_c = min(row, kv_len - 1);
      ke[h] = Keb[row_c * Hkv];
      ve[h] = Veb[row_c * Hkv];
#pragma unroll
      for (int lo = 0; lo < 2; ++lo) {
        const long long r =
            row_c * kv_rowstride + ((tid & 7) | (lo << 3)) * 8;
        kpre[2 * h + lo] = *(const i32x2*)(Kb + r);
        const i32x2 vv = *(const i32x2*)(Vb + r);
        // code 0 is +0: rows at or past kv_len are staged as zeros
        vpre[2 * h + lo] = (row < kv_len) ? vv : i32x2{0, 0};
      }
    }
  }
  __device__ __forceinline__ s16x8 k(int i) const {
    return kv8_dequant_bf16(kpre[i], kv8_scale(ke[i >> 1]));
  }
  __device__ __forceinline__ s16x8 v(int i) const {
    return kv8_dequant_bf16(vpre[i], kv8_scale(ve[i >> 1]));
  }
};

#define APPEND_KERNEL attn_append_kernel
#define APPEND_FP8 0
#include "attn_append_body.h"
#undef APPEND_KERNEL
#undef APPEND_FP8

#define APPEND_KERNEL attn_append_fp8_kernel
#define APPEND_FP8 1
#include "attn_append_body.h"
#undef APPEND_KERNEL
#undef APPEND_FP8

extern "C" void attn_append_launch(const void* Q, const void* Kc,
                                   const void* Vc, void* O,
                                   const int* slot_ids, const int* q_start,
                                   const int* q_lens, int n, int Sq, int Hq,
                                   int Hkv, int slots, int S_max,
                                   float scale, hipStream_t stream) {
  dim3 grid(Sq / BM, n * Hq);
  hipLaunchKernelGGL(attn_append_kernel, grid, dim3(256), 0, stream,
                     (const unsigned short*)Q, (const unsigned short*)Kc,
                     (const unsigned short*)Vc, (unsigned short*)O, slot_ids,
                     q_start, q_lens, Sq, Hq, Hkv, slots, S_max, scale);
}

extern "C" void attn_append_fp8_launch(const void* Q, const void* Kc,
                                       const void* Vc, const void* Ke,
                                       const void* Ve, void* O,
                                       const int* slot_ids,
                                       const int* q_start, const int* q_lens,
                                       int n, int Sq, int Hq, int Hkv,
                                       int slots, int S_max, float scale,
                                       hipStream_t stream) {
  dim3 grid(Sq / BM, n * Hq);
  hipLaunchKernelGGL(attn_append_fp8_kernel, grid, dim3(256), 0, stream,
                     (const unsigned short*)Q, (const unsigned char*)Kc,
                     (const unsigned char*)Vc, (const unsigned char*)Ke,
                     (const unsigned char*)Ve, (unsigned short*)O, slot_ids,
                     q_start, q_lens, Sq, Hq, Hkv, slots, S_max, scale);
}
