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
#include "attn_append.h"
#include "common.h"

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

extern "C" __global__ __launch_bounds__(256, 2) void attn_append_kernel(
    const unsigned short* __restrict__ Q, const unsigned short* __restrict__ Kc,
    const unsigned short* __restrict__ Vc, unsigned short* __restrict__ O,
    const int* __restrict__ slot_ids, const int* __restrict__ q_start,
    const int* __restrict__ q_lens, int Sq, int Hq, int Hkv, int slots,
    int S_max, float scale) {
  __shared__ unsigned short k_lds[BN * ATT_D];    // [kv][d], swizzled, 16KB
  __shared__ unsigned short vt_lds[ATT_D * BN];   // [d][kv], swizzled, 16KB

  const int qt = gridDim.x - 1 - blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / Hq;
  const int qh = bh % Hq;
  const int kvh = qh / (Hq / Hkv);
  const int qbase = qt * BM;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;               // wave id: q rows [16w, 16w+16)
  const int lrow = lane & 15;           // q column owned by this lane
  const int lgrp = lane >> 4;

  // Per-sequence scalars (SGPRs).  An index the cache cannot hold (slot
  // outside [0, slots), negative start) makes the sequence empty instead
  // of an out-of-bounds read.
  const int slot = __builtin_amdgcn_readfirstlane(slot_ids[b]);
  const int qs = __builtin_amdgcn_readfirstlane(q_start[b]);
  int ql = __builtin_amdgcn_readfirstlane(q_lens[b]);
  ql = min(max(ql, 0), Sq);
  if (slot < 0 || slot >= slots || qs < 0) ql = 0;
  const int kv_len = (int)min((long long)qs + ql, (long long)S_max);

  const long long q_rowstride = (long long)Hq * ATT_D;
  const long long kv_rowstride = (long long)Hkv * ATT_D;
  const unsigned short* Qb = Q + ((long long)b * Sq * Hq + qh) * ATT_D;
  unsigned short* Ob = O + ((long long)b * Sq * Hq + qh) * ATT_D;

  if (qbase >= ql) {
    // Padding-only tile (every tile of an empty sequence): finite output,
    // no cache row read.  Thread t zeroes chunk t&15 of rows (t>>4)+16i.
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = qbase + (tid >> 4) + 16 * i;
      *(s16x8*)(Ob + (long long)row * q_rowstride + (tid & 15) * 8) =
          s16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    return;
  }
  // From here ql >= 1, so kv_len >= 1 and kv row 0 is visible to every
  // row of the tile: no softmax column ends empty.

  const unsigned short* Kb =
      Kc + ((long long)slot * S_max * Hkv + kvh) * ATT_D;
  const unsigned short* Vb =
      Vc + ((long long)slot * S_max * Hkv + kvh) * ATT_D;

  // Q as B-fragments: B[k=d][n=q]: lane holds Q[q=lrow][d=ks*32+lgrp*8+j].
  s16x8 q_b[4];
  {
    const int qrow = qbase + 16 * w + lrow;
    const unsigned short* src = Qb + (long long)qrow * q_rowstride;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      q_b[ks] = *(const s16x8*)(src + ks * 32 + lgrp * 8);
  }

  // Per-lane softmax state for q column lrow (replicated across lgrp).
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 o_t[8];  // O^T: C[row=d=ct*16+lgrp*4+r][col=q=lrow]
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) o_t[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  // kv rows the tile can see: up to the diagonal of its last row, and
  // never past kv_len.
  const int kv_end = (int)min((long long)kv_len, (long long)qs + qbase + BM);
  const int n_kv_tiles = (kv_end + BN - 1) / BN;

  s16x8 kpre[4], vpre[4];
  append_load_tile(Kb, Vb, kv_rowstride, 0, kv_len, tid, kpre, vpre);

  // Absolute positions, capped at S_max: kv < kv_len <= S_max, so a cap
  // there changes no comparison and keeps them 32-bit.
  const int my_q = qbase + 16 * w + lrow;  // row of the chunk
  const int my_pos = (int)min((long long)qs + my_q, (long long)S_max);
  const int wave_pos0 =
      (int)min((long long)qs + qbase + 16 * w, (long long)S_max);
  for (int kt = 0; kt < n_kv_tiles; ++kt) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int s_ch = (tid & 7) | ((i & 1) << 3);
      int s_row = (tid >> 3) | ((i >> 1) << 5);
      *(s16x8*)((char*)k_lds + swz(s_row * 256 + s_ch * 16, s_row)) =
          kpre[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int d = s_ch * 8 + j;
        *(unsigned short*)((char*)vt_lds + swzT(d * 128 + s_row * 2, d)) =
            (unsigned short)vpre[i][j];
      }
    }
    __syncthreads();
    if (kt + 1 < n_kv_tiles)
      append_load_tile(Kb, Vb, kv_rowstride, (kt + 1) * BN, kv_len, tid,
                       kpre, vpre);
    const int kvbase = kt * BN;

    // ---- S^T = scale * K Q^T : 64 kv rows x 16 q cols for this wave.
    f32x4 st_acc[4];
#pragma unroll
    for (int kv4 = 0; kv4 < 4; ++kv4)
      st_acc[kv4] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int kv4 = 0; kv4 < 4; ++kv4) {
        int krow = kv4 * 16 + lrow;
        s16x8 a_k = *(const s16x8*)((char*)k_lds +
            swz(krow * 256 + (ks * 32 + lgrp * 8) * 2, krow));
        st_acc[kv4] = MFMA_BF16(as_bf16x8(a_k), as_bf16x8(q_b[ks]),
                                st_acc[kv4]);
      }

    // ---- mask + in-register column softmax (q = lrow on every lane).
    // The diagonal is at the absolute position; the tile needs the mask
    // when it reaches past the wave's first position or past kv_len.
    const bool need_mask =
        (kvbase + BN - 1 > wave_pos0) || (kvbase + BN > kv_len);
    float mx = -INFINITY;
#pragma unroll
    for (int kv4 = 0; kv4 < 4; ++kv4)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = st_acc[kv4][r] * scale;
        if (need_mask) {
          int kv = kvbase + kv4 * 16 + lgrp * 4 + r;
          if (kv > my_pos || kv >= kv_len) s = -INFINITY;
        }
        st_acc[kv4][r] = s;
        mx = fmaxf(mx, s);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float m_new = fmaxf(m_run, mx);
    float m_safe = (m_new == -INFINITY) ? 0.f : m_new;
    float corr = (m_run == -INFINITY) ? 0.f : __expf(m_run - m_safe);
    m_run = m_new;
    float rs = 0.f;
#pragma unroll
    for (int kv4 = 0; kv4 < 4; ++kv4)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float e = (st_acc[kv4][r] == -INFINITY)
                      ? 0.f : __expf(st_acc[kv4][r] - m_safe);
        st_acc[kv4][r] = e;  // P^T stays in the S registers
        rs += e;
      }
    rs += __shfl_xor(rs, 16, 64);
    rs += __shfl_xor(rs, 32, 64);
    l_run = l_run * corr + rs;
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) o_t[ct][r] *= corr;

    // ---- P^T -> B-fragments via cross-lane shuffles (parent's recipe).
    s16x8 p_b[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int src = (2 * (lgrp & 1) + (j >> 2)) * 16 + lrow;
        float v0 = __shfl(st_acc[2 * ks][j & 3], src, 64);
        float v1 = __shfl(st_acc[2 * ks + 1][j & 3], src, 64);
        p_b[ks][j] = (short)f2bf_trunc((lgrp >> 1) ? v1 : v0);
      }
    }

    // ---- O^T += V^T P^T : A from vt_lds.
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        int vrow = ct * 16 + lrow;
        s16x8 a_vt = *(const s16x8*)((char*)vt_lds +
            swzT(vrow * 128 + (ks * 32 + lgrp * 8) * 2, vrow));
        o_t[ct] = MFMA_BF16(as_bf16x8(a_vt), as_bf16x8(p_b[ks]), o_t[ct]);
      }
  }

  // ---- epilogue: O[q][d] = O^T[d][q] / l (s16x4 stores, d block
  // ct*16 + lgrp*4).
  const float inv_l = (l_run > 0.f) ? 1.f / l_run : 0.f;
  unsigned short* orow = Ob + (long long)my_q * q_rowstride;
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) {
    s16x4 ov;
#pragma unroll
    for (int r = 0; r < 4; ++r) ov[r] = (short)f2bf(o_t[ct][r] * inv_l);
    *(s16x4*)(orow + ct * 16 + lgrp * 4) = ov;
  }
}

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
