// Flash-attention backward v3 — 32x32 MFMA deep-pipeline kernels.
//
// Round-2 rewrite of dkv/dq on the v3 structure (see attention_fwd_v3):
// tr reads instead of transposed scatter staging, permlane P/dS
// redistribution instead of LDS roundtrips, exp2-domain softmax.
//
// dkv: computes S UNSWAPPED (S[q][kv] = Q K^T with K as the B operand)
// so the MFMA C-layout puts each lane's OWN kv column on the lane and q
// on the registers; P^T / dS^T A-fragments for the dV/dK accumulation
// then come from the SAME cvt_pk+permlane half-swap as the forward's
// P^T B-fragments — the round-1 dkv LDS roundtrip (p_lds/ds_lds, two
// swizzled write+read passes per tile) disappears entirely.  K and V
// rows live in per-wave registers for the whole kernel (one block per
// 128 kv rows); Q/dO tiles of 32 rows are staged per iteration in a
// bank-swizzled subtile layout serving both b128 row-fragments and
// hardware-transpose column-fragments.
//
// dq: a structural clone of the forward (block per 128 q rows, kv tiles
// of 64 staged by global_load_lds, swapped S^T), with a second MFMA
// pass for dP^T = V dO^T and the output pass dQ^T = K^T dS^T whose
// A-fragments are tr reads of the K tile and B-fragments the permlane
// pack of dS^T.
//
// Math (identical to v1, attention_bwd.hip):
//   P = exp(scale*QK^T - lse); dP = dO V^T; dS = P*(dP - Dvec);
//   dV += P^T dO; dK += scale * dS^T Q; dQ = scale * dS K.
#include "attn_launch.h"
#include "attn_v3.h"

// Q/dO tile layout for dkv: [32 q][128 d] in vsub subtiles with an
// extra XOR on the d-chunk keyed by q>>2 — without it, b128 row-reads
// (32 q rows at one fixed d-chunk) land 8-way on the same bank set.
__device__ __forceinline__ int vsubz(int q, int d) {
  return (((q >> 2) << 3) + ((d >> 4) ^ ((q >> 2) & 7))) * 64 +
         ((q & 3) << 4) + (d & 15);
}

// ---------------------------------------------------------------------------
// dkv kernel.  Grid: (S/128, B*Hkv); 256 threads (4 waves); wave w owns
// kv rows [kvb+32w, kvb+32w+32).
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256, 2) void attn_bwd_dkv_v3_kernel(
    const unsigned short* __restrict__ Q, const unsigned short* __restrict__ K,
    const unsigned short* __restrict__ V, const unsigned short* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ Dvec,
    unsigned short* __restrict__ dK, unsigned short* __restrict__ dV, int B,
    int S, int Hq, int Hkv, float scale, int causal) {
  __shared__ unsigned short q_lds[32 * ATT_D];     // 8 KB, swzK16 layout
  __shared__ unsigned short do_lds[32 * ATT_D];    // 8 KB
  __shared__ unsigned short k_own[128 * ATT_D];    // 32 KB, block's K rows
  __shared__ unsigned short v_own[128 * ATT_D];    // 32 KB, block's V rows
  // (80 KB total: exactly two blocks per CU; lse/Dvec read from L2)

  const int kt = blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / Hkv;
  const int kvh = bh % Hkv;
  const int group = Hq / Hkv;
  const int kvb = kt * 128;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int col = lane & 31;
  const int h = lane >> 5;
  const int g = lane >> 4;
  const int lw = lane & 15;

  const long long q_rowstride = (long long)Hq * ATT_D;
  const long long kv_rowstride = (long long)Hkv * ATT_D;
  const unsigned short* Kb = K + ((long long)b * S * Hkv + kvh) * ATT_D;
  const unsigned short* Vb = V + ((long long)b * S * Hkv + kvh) * ATT_D;

  const int my_kv = kvb + 32 * w + col;

  // Block's K/V rows staged ONCE into LDS (vsubz layout): keeping them
  // in per-wave registers (64 VGPRs) spilled.  K is pre-scaled by
  // scale*log2(e) during staging (it feeds ONLY the S pass; dK
  // accumulates separately).  V raw.
  const float ksc = scale * 1.44269504088896340736f;
  {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int c = tid * 8 + i;  // 2048 16B chunks in a [128][128] tile
      int kr = c >> 4;
      int dch = (c & 15) * 8;
      long long src = (long long)(kvb + kr) * kv_rowstride + dch;
      s16x8 raw = *(const s16x8*)(Kb + src);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        raw[j] = (short)f2bf(bf2f((unsigned short)raw[j]) * ksc);
      int koff = kr * 256 + (((dch >> 3) ^ (kr & 15)) << 4);
      *(s16x8*)((char*)k_own + koff) = raw;
      *(s16x8*)((char*)v_own + koff) = *(const s16x8*)(Vb + src);
    }
  }

  f32x16 dv_acc[4], dk_acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dv_acc[dt][r] = 0.f;
      dk_acc[dt][r] = 0.f;
    }

  const int qt0 = causal ? kvb / 32 : 0;
  const int n_qt = S / 32;

  for (int gi = 0; gi < group; ++gi) {
    const int qh = kvh * group + gi;
    const unsigned short* Qb = Q + ((long long)b * S * Hq + qh) * ATT_D;
    const unsigned short* dOb = dO + ((long long)b * S * Hq + qh) * ATT_D;
    const float* lse_b = lse + ((long long)b * Hq + qh) * S;
    const float* dvec_b = Dvec + ((long long)b * Hq + qh) * S;

    for (int qt = qt0; qt < n_qt; ++qt) {
      const int qbase = qt * 32;
      __syncthreads();
      // ---- stage Q/dO tile (2 x 16B chunks per thread) + lse/Dvec.
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        int c = tid * 2 + i;
        int qr = c >> 4;
        int dch = (c & 15) * 8;
        long long src = (long long)(qbase + qr) * q_rowstride + dch;
        int off = qr * 256 + (((dch >> 3) ^ (qr & 15)) << 4);
        *(s16x8*)((char*)q_lds + off) = *(const s16x8*)(Qb + src);
        *(s16x8*)((char*)do_lds + off) = *(const s16x8*)(dOb + src);
      }
      __syncthreads();
      // causal: this wave's kv rows see q tiles >= its diagonal only.
      if (causal && qbase + 31 < kvb + 32 * w) continue;

      // ---- S[q][kv_own] and dP[q][kv_own]: A = Q/dO row-fragments
      // from LDS, B = K'/V register fragments.  Two interleaved
      // accumulator chains.
      f32x16 st, dpt;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[r] = 0.f;
        dpt[r] = 0.f;
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        s16x8 aq = *(const s16x8*)(
            (char*)q_lds + swzK16(col * 256 + (ks * 2 + h) * 16, col));
        s16x8 kfr = *(const s16x8*)(
            (char*)k_own +
            swzK16((32 * w + col) * 256 + (ks * 2 + h) * 16, 32 * w + col));
        st = MFMA32V3(as_bf16x8(aq), as_bf16x8(kfr), st);
        s16x8 ad = *(const s16x8*)(
            (char*)do_lds + swzK16(col * 256 + (ks * 2 + h) * 16, col));
        s16x8 vfr = *(const s16x8*)(
            (char*)v_own +
            swzK16((32 * w + col) * 256 + (ks * 2 + h) * 16, 32 * w + col));
        dpt = MFMA32V3(as_bf16x8(ad), as_bf16x8(vfr), dpt);
      }
      __builtin_amdgcn_s_setprio(0);

      // ---- P = exp2(S' - lse'); dS = P * (dP - Dvec).  q is the
      // register row, kv the lane column; causal mask only on the
      // diagonal q-tile band.
      const bool need_mask = causal && qbase < kvb + 128;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ql = (r & 3) + ((r >> 2) << 3) + (h << 2);
        float lv = lse_b[qbase + ql];
        float l2 = (lv == -INFINITY) ? 3.0e37f
                                     : lv * 1.44269504088896340736f;
        float p = exp2f(st[r] - l2);
        if (need_mask && qbase + ql < my_kv) p = 0.f;
        st[r] = p;
        dpt[r] = p * (dpt[r] - dvec_b[qbase + ql]);
      }

      // ---- dV += P^T dO ; dK += dS^T Q.  A-fragments come straight
      // from the C-layout registers via the permlane half-swap pack;
      // B-fragments are tr reads of the dO / Q tiles.
      s16x8 pa, da;
      tr4 t0, t1;
#define DKV_TRA(base, qv, dv)                                             \
  ((base) + (qv) * 256 + ((((dv) >> 3) ^ ((qv) & 15)) << 4) +             \
   (((dv) & 7) << 1))
#define DKV_TR_ISSUE(lds_base, ks)                                        \
  {                                                                       \
    int q_s = (ks) * 16 + ((g >> 1) << 3) + (lw >> 2);                    \
    int d_s = ((g & 1) << 4) + ((lw & 3) << 2);                           \
    unsigned base = (unsigned)(size_t)((char*)(lds_base));                \
    ds_tr4_issue(&t0, DKV_TRA(base, q_s, d_s),                            \
                 DKV_TRA(base, q_s + 4, d_s),                             \
                 DKV_TRA(base, q_s, 32 + d_s),                            \
                 DKV_TRA(base, q_s + 4, 32 + d_s));                       \
    ds_tr4_issue(&t1, DKV_TRA(base, q_s, 64 + d_s),                       \
                 DKV_TRA(base, q_s + 4, 64 + d_s),                        \
                 DKV_TRA(base, q_s, 96 + d_s),                            \
                 DKV_TRA(base, q_s + 4, 96 + d_s));                       \
  }
#define DKV_MFMA(acc, afrag)                                              \
  {                                                                       \
    union { unsigned long long u[2]; s16x8 v; } bf;                       \
    __builtin_amdgcn_s_setprio(1);                                        \
    bf.u[0] = t0.d[0];                                                    \
    bf.u[1] = t0.d[1];                                                    \
    acc[0] = MFMA32V3(as_bf16x8(afrag), as_bf16x8(bf.v), acc[0]);         \
    bf.u[0] = t0.d[2];                                                    \
    bf.u[1] = t0.d[3];                                                    \
    acc[1] = MFMA32V3(as_bf16x8(afrag), as_bf16x8(bf.v), acc[1]);         \
    bf.u[0] = t1.d[0];                                                    \
    bf.u[1] = t1.d[1];                                                    \
    acc[2] = MFMA32V3(as_bf16x8(afrag), as_bf16x8(bf.v), acc[2]);         \
    bf.u[0] = t1.d[2];                                                    \
    bf.u[1] = t1.d[3];                                                    \
    acc[3] = MFMA32V3(as_bf16x8(afrag), as_bf16x8(bf.v), acc[3]);         \
    __builtin_amdgcn_s_setprio(0);                                        \
  }
      // ks = 0: q rows 0..15; ks = 1: q rows 16..31.
      DKV_TR_ISSUE(do_lds, 0);
      V3_PACK1(pa, st, 0);
      lgkm_wait0_bind2(&t0, &t1);
      DKV_MFMA(dv_acc, pa);
      DKV_TR_ISSUE(do_lds, 1);
      V3_PACK1(pa, st, 1);
      lgkm_wait0_bind2(&t0, &t1);
      DKV_MFMA(dv_acc, pa);
      DKV_TR_ISSUE(q_lds, 0);
      V3_PACK1(da, dpt, 0);
      lgkm_wait0_bind2(&t0, &t1);
      DKV_MFMA(dk_acc, da);
      DKV_TR_ISSUE(q_lds, 1);
      V3_PACK1(da, dpt, 1);
      lgkm_wait0_bind2(&t0, &t1);
      DKV_MFMA(dk_acc, da);
    }
    // group loop: reset nothing (dv/dk keep accumulating); barrier
    // protects the next gi's staging via loop-top __syncthreads.
  }

  // ---- epilogue: C-layout [kv row][d col]; dK gets the outer scale.
  unsigned short* dKb = dK + ((long long)b * S * Hkv + kvh) * ATT_D;
  unsigned short* dVb = dV + ((long long)b * S * Hkv + kvh) * ATT_D;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kvrow = kvb + 32 * w + (r & 3) + ((r >> 2) << 3) + (h << 2);
    unsigned short* krow = dKb + (long long)kvrow * kv_rowstride;
    unsigned short* vrow = dVb + (long long)kvrow * kv_rowstride;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      krow[dt * 32 + col] = f2bf(dk_acc[dt][r] * scale);
      vrow[dt * 32 + col] = f2bf(dv_acc[dt][r]);
    }
  }
}

// A wave-uniform pointer pinned to scalar registers: loads through
// `uniform_ptr(p) + lane_offset32` take the scalar-base + 32-bit
// lane-offset form and need no 64-bit per-lane address registers.
typedef const __attribute__((address_space(1))) char* gptr_t;
__device__ __forceinline__ gptr_t uniform_ptr(const void* p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (gptr_t)(((unsigned long long)hi << 32) | lo);
}
typedef const __attribute__((address_space(1))) s16x8* g_s16x8_t;
typedef const __attribute__((address_space(1))) f32x4* g_f32x4_t;

// ---------------------------------------------------------------------------
// Pipelined dkv kernel: the same MFMA sequence, LDS layouts and
// accumulation order as attn_bwd_dkv_v3_kernel (dK/dV are bit-identical);
// only the schedule of the memory traffic differs.
//
//  * Q/dO staging is split into a global->register load and a
//    register->LDS write one iteration apart: the loads of tile t+1 are
//    issued right after the second barrier of tile t (4 x 16 B per
//    thread, 16 VGPRs) and land during tile t's MFMAs; the ds_write runs
//    at the top of iteration t+1 after the first barrier.  The prefetch
//    crosses the q-head boundary; a prologue loads the first tile.  LDS
//    stays at 80 KB.
//  * lse and Dvec ([B,Hq,S], contiguous in s) come in as 4 + 4 float4
//    loads per lane, issued before the first barrier and consumed after
//    the S/dP MFMA chain.  They are issued BEFORE the tile prefetch so
//    that the counted vmcnt wait in front of the softmax leaves the four
//    prefetch loads in flight.
//  * heavy_first swaps the grid axes (grid = (B*Hkv, S/128)): blocks are
//    dispatched in descending causal work order, kt = 0 of every
//    (b, kv-head) first.
//
// Every wave still reaches both barriers of every iteration; the causal
// skip drops only compute (a skipping wave still stages and prefetches).
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256, 2) void attn_bwd_dkv_v3p_kernel(
    const unsigned short* __restrict__ Q, const unsigned short* __restrict__ K,
    const unsigned short* __restrict__ V, const unsigned short* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ Dvec,
    unsigned short* __restrict__ dK, unsigned short* __restrict__ dV, int B,
    int S, int Hq, int Hkv, float scale, int causal, int heavy_first) {
  // One array so every tile sits at a compile-time offset from the
  // others (tr reads of do_lds and of the second 16 q rows then reuse
  // the q_lds address registers through the DS offset field).  The tiles
  // and their internal layouts are those of attn_bwd_dkv_v3_kernel.
  // 80 KB total: exactly two blocks per CU — no second Q/dO buffer.
  __shared__ unsigned short lds[(2 * 32 + 2 * 128) * ATT_D];
  unsigned short* q_lds = lds;                    // 8 KB, swzK16 layout
  unsigned short* do_lds = lds + 32 * ATT_D;      // 8 KB
  unsigned short* k_own = lds + 64 * ATT_D;       // 32 KB, block's K rows
  unsigned short* v_own = lds + 192 * ATT_D;      // 32 KB, block's V rows

  const int kt = heavy_first ? blockIdx.y : blockIdx.x;
  const int bh = heavy_first ? blockIdx.x : blockIdx.y;
  const int b = bh / Hkv;
  const int kvh = bh % Hkv;
  const int group = Hq / Hkv;
  const int kvb = kt * 128;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int col = lane & 31;
  const int h = lane >> 5;
  const int g = lane >> 4;
  const int lw = lane & 15;

  const long long q_rowstride = (long long)Hq * ATT_D;
  const long long kv_rowstride = (long long)Hkv * ATT_D;
  const unsigned short* Kb = K + ((long long)b * S * Hkv + kvh) * ATT_D;
  const unsigned short* Vb = V + ((long long)b * S * Hkv + kvh) * ATT_D;

  const int my_kv = kvb + 32 * w + col;

  const int qt0 = causal ? kvb / 32 : 0;
  const int n_qt = S / 32;

  // The eight tr-read addresses of q rows 0..15 in q_lds (DKV_TR_ISSUE
  // with ks = 0); the other three fragment sets are constant offsets.
  unsigned tra[8];
  {
    const int q_s = ((g >> 1) << 3) + (lw >> 2);
    const int d_s = ((g & 1) << 4) + ((lw & 3) << 2);
    const unsigned base = (unsigned)(size_t)((char*)q_lds);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      tra[i] = DKV_TRA(base, q_s + 4 * (i & 1), 32 * (i >> 1) + d_s);
  }
#define DKVP_TR_ISSUE(off)                                                \
  {                                                                       \
    ds_tr4_issue_off<(off)>(&t0, tra[0], tra[1], tra[2], tra[3]);         \
    ds_tr4_issue_off<(off)>(&t1, tra[4], tra[5], tra[6], tra[7]);         \
  }

  // Row-fragment byte offsets at k-step 0: swzK16(col*256 + h*16, col) in
  // the Q/dO tile and the same for row 32w+col of K/V.  k-step ks sits at
  // offset ^ (ks << 5): (2ks + h) ^ x == (h ^ x) ^ 2ks, and neither the
  // row term (bits >= 8) nor 8192w touches bits 5..7.
  const unsigned frag_q = (unsigned)swzK16(col * 256 + h * 16, col);
  const unsigned frag_k = frag_q + (unsigned)w * 8192u;

  // Prefetch registers for the next Q/dO tile (2 x 16 B chunks each).
  s16x8 pq[2], pd[2];
  // Per-lane byte offset of this thread's two adjacent 16 B chunks inside
  // a Q/dO tile; the tile base is wave-uniform (scalar base + 32-bit lane
  // offset addressing keeps the loads off 64-bit address registers).
  const unsigned st_off =
      (unsigned)(((tid * 2) >> 4) * q_rowstride + ((tid * 2) & 15) * 8) * 2u;
  const unsigned row_off = (unsigned)h * 16u;  // lse/Dvec: 4 floats per half
#define DKVP_PREFETCH(qh_, qbase_)                                        \
  {                                                                       \
    const long long tb = ((long long)b * S * Hq + (qh_)) * ATT_D +        \
                         (long long)(qbase_) * q_rowstride;               \
    gptr_t qsrc = uniform_ptr(Q + tb) + st_off;                           \
    gptr_t dsrc = uniform_ptr(dO + tb) + st_off;                          \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                       \
      pq[i] = *(g_s16x8_t)(qsrc + 16 * i);                                \
      pd[i] = *(g_s16x8_t)(dsrc + 16 * i);                                \
    }                                                                     \
  }
  // Prologue: first tile of the first q head, in flight during the K/V
  // staging below.
  DKVP_PREFETCH(kvh * group, qt0 * 32);

  // Block's K/V rows staged ONCE into LDS, K pre-scaled by
  // scale*log2(e) (see attn_bwd_dkv_v3_kernel).
  const float ksc = scale * 1.44269504088896340736f;
  {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int c = tid * 8 + i;  // 2048 16B chunks in a [128][128] tile
      int kr = c >> 4;
      int dch = (c & 15) * 8;
      long long src = (long long)(kvb + kr) * kv_rowstride + dch;
      s16x8 raw = *(const s16x8*)(Kb + src);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        raw[j] = (short)f2bf(bf2f((unsigned short)raw[j]) * ksc);
      int koff = kr * 256 + (((dch >> 3) ^ (kr & 15)) << 4);
      *(s16x8*)((char*)k_own + koff) = raw;
      *(s16x8*)((char*)v_own + koff) = *(const s16x8*)(Vb + src);
    }
  }

  f32x16 dv_acc[4], dk_acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dv_acc[dt][r] = 0.f;
      dk_acc[dt][r] = 0.f;
    }

  for (int gi = 0; gi < group; ++gi) {
    const int qh = kvh * group + gi;
    const float* lse_b = lse + ((long long)b * Hq + qh) * S;
    const float* dvec_b = Dvec + ((long long)b * Hq + qh) * S;

    for (int qt = qt0; qt < n_qt; ++qt) {
      const int qbase = qt * 32;
      // ---- lse/Dvec rows of this lane: ql = (r&3) + 8(r>>2) + 4h is
      // four runs of four consecutive q rows -> 4 + 4 float4 loads.
      f32x4 lv4[4], dv4[4];
      gptr_t lse_t = uniform_ptr(lse_b + qbase);
      gptr_t dvec_t = uniform_ptr(dvec_b + qbase);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lv4[j] = *(g_f32x4_t)(lse_t + 32 * j + row_off);
        dv4[j] = *(g_f32x4_t)(dvec_t + 32 * j + row_off);
      }
      __syncthreads();
      // ---- write the prefetched Q/dO tile to LDS.
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        int c = tid * 2 + i;
        int qr = c >> 4;
        int dch = (c & 15) * 8;
        int off = qr * 256 + (((dch >> 3) ^ (qr & 15)) << 4);
        *(s16x8*)((char*)q_lds + off) = pq[i];
        *(s16x8*)((char*)do_lds + off) = pd[i];
      }
      __syncthreads();
      // ---- issue the next tile's loads (next q tile, or the first tile
      // of the next q head); they complete under this tile's MFMAs.  The
      // loads are unconditional so that the wait in front of the softmax
      // can be a counted vmcnt(4) on every path: the block's last
      // iteration re-reads its own tile (16 KB, unused) instead.
      {
        int nqt = qt + 1, ngi = gi;
        if (nqt == n_qt) {
          nqt = qt0;
          ngi = gi + 1;
        }
        if (ngi == group) {
          nqt = qt;
          ngi = gi;
        }
        DKVP_PREFETCH(kvh * group + ngi, nqt * 32);
      }
      // causal: this wave's kv rows see q tiles >= its diagonal only.
      if (causal && qbase + 31 < kvb + 32 * w) {
        // Name the lse/Dvec values on this path too: with a use on both
        // paths the loads stay above the barriers, ahead of the prefetch
        // in the vmcnt queue, instead of being sunk into the compute path.
#pragma unroll
        for (int j = 0; j < 4; ++j)
          asm volatile("" ::"v"(lv4[j]), "v"(dv4[j]));
        continue;
      }

      // ---- S[q][kv_own] and dP[q][kv_own] (two interleaved chains).
      f32x16 st, dpt;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[r] = 0.f;
        dpt[r] = 0.f;
      }
      // Fragment addresses are rebuilt per k-step from two lane bases by
      // one XOR each (frag_q/frag_k above) instead of being kept in 16
      // loop-invariant registers; the empty asm makes the bases opaque
      // per iteration so that they are not hoisted back out.
      unsigned fq = frag_q, fk = frag_k;
      asm volatile("" : "+v"(fq), "+v"(fk));
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const unsigned oq = fq ^ (ks << 5), ok = fk ^ (ks << 5);
        s16x8 aq = *(const s16x8*)((char*)q_lds + oq);
        s16x8 kfr = *(const s16x8*)((char*)k_own + ok);
        st = MFMA32V3(as_bf16x8(aq), as_bf16x8(kfr), st);
        s16x8 ad = *(const s16x8*)((char*)do_lds + oq);
        s16x8 vfr = *(const s16x8*)((char*)v_own + ok);
        dpt = MFMA32V3(as_bf16x8(ad), as_bf16x8(vfr), dpt);
      }
      // Pin the interleave: two fragment pairs are read ahead, then each
      // MFMA is followed by the reads of the pair two MFMAs later, so a
      // read always has one full MFMA to land (three 8-register pairs).
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);  // 4 DS reads
#pragma unroll
      for (int i = 0; i < 14; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // 2 DS reads
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      __builtin_amdgcn_s_setprio(0);

      // ---- P = exp2(S' - lse'); dS = P * (dP - Dvec): the same guard,
      // scaling and mask as attn_bwd_dkv_v3_kernel.
      const bool need_mask = causal && qbase < kvb + 128;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ql = (r & 3) + ((r >> 2) << 3) + (h << 2);
        float lv = lv4[r >> 2][r & 3];
        float l2 = (lv == -INFINITY) ? 3.0e37f
                                     : lv * 1.44269504088896340736f;
        float p = exp2f(st[r] - l2);
        if (need_mask && qbase + ql < my_kv) p = 0.f;
        st[r] = p;
        dpt[r] = p * (dpt[r] - dv4[r >> 2][r & 3]);
      }

      // ---- dV += P^T dO ; dK += dS^T Q (as attn_bwd_dkv_v3_kernel).
      s16x8 pa, da;
      tr4 t0, t1;
      // tile byte offsets: do_lds = q_lds + 8192; q rows 16..31 = +4096.
      DKVP_TR_ISSUE(8192);
      V3_PACK1(pa, st, 0);
      lgkm_wait0_bind2(&t0, &t1);
      DKV_MFMA(dv_acc, pa);
      DKVP_TR_ISSUE(8192 + 4096);
      V3_PACK1(pa, st, 1);
      lgkm_wait0_bind2(&t0, &t1);
      DKV_MFMA(dv_acc, pa);
      DKVP_TR_ISSUE(0);
      V3_PACK1(da, dpt, 0);
      lgkm_wait0_bind2(&t0, &t1);
      DKV_MFMA(dk_acc, da);
      DKVP_TR_ISSUE(4096);
      V3_PACK1(da, dpt, 1);
      lgkm_wait0_bind2(&t0, &t1);
      DKV_MFMA(dk_acc, da);
    }
  }
#undef DKVP_PREFETCH
#undef DKVP_TR_ISSUE

  // ---- epilogue: C-layout [kv row][d col]; dK gets the outer scale.
  unsigned short* dKb = dK + ((long long)b * S * Hkv + kvh) * ATT_D;
  unsigned short* dVb = dV + ((long long)b * S * Hkv + kvh) * ATT_D;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kvrow = kvb + 32 * w + (r & 3) + ((r >> 2) << 3) + (h << 2);
    unsigned short* krow = dKb + (long long)kvrow * kv_rowstride;
    unsigned short* vrow = dVb + (long long)kvrow * kv_rowstride;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      krow[dt * 32 + col] = f2bf(dk_acc[dt][r] * scale);
      vrow[dt * 32 + col] = f2bf(dv_acc[dt][r]);
    }
  }
}

// ---------------------------------------------------------------------------
// dq kernel.  Grid: (S/128, B*Hq); 256 threads (4 waves); wave w owns q
// rows [qb+32w, qb+32w+32).  kv tiles of 64 staged by global_load_lds
// into the forward's linear+swzK16 layout (K is read both as b128
// row-fragments for S^T and as tr column-fragments for dQ^T = K^T dS^T).
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256, 2) void attn_bwd_dq_v3_kernel(
    const unsigned short* __restrict__ Q, const unsigned short* __restrict__ K,
    const unsigned short* __restrict__ V, const unsigned short* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ Dvec,
    unsigned short* __restrict__ dQ, int B, int S, int Hq, int Hkv,
    float scale, int causal) {
  __shared__ unsigned short k_lds[2][64 * ATT_D];  // 2 x 16 KB
  __shared__ unsigned short v_lds[2][64 * ATT_D];  // 2 x 16 KB

  // Paired causal grid (see attention_fwd_v3): heavy q-tile then light
  // one per block, staging pipeline continuous across the boundary.
  const int nq = S / 128;
  const bool paired = causal && (int)gridDim.x * 2 == nq;
  const int qtA = paired ? nq - 1 - (int)blockIdx.x
                         : (int)gridDim.x - 1 - (int)blockIdx.x;
  const int qtB = paired ? (int)blockIdx.x : 0;
  const int bh = blockIdx.y;
  const int b = bh / Hq;
  const int qh = bh % Hq;
  const int kvh = qh / (Hq / Hkv);
  int qbase = qtA * 128;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int col = lane & 31;
  const int h = lane >> 5;
  const int g = lane >> 4;
  const int lw = lane & 15;

  const long long q_rowstride = (long long)Hq * ATT_D;
  const long long kv_rowstride = (long long)Hkv * ATT_D;
  const unsigned short* Qb = Q + ((long long)b * S * Hq + qh) * ATT_D;
  const unsigned short* Kb = K + ((long long)b * S * Hkv + kvh) * ATT_D;
  const unsigned short* Vb = V + ((long long)b * S * Hkv + kvh) * ATT_D;
  const unsigned short* dOb = dO + ((long long)b * S * Hq + qh) * ATT_D;

  int my_q = qbase + 32 * w + col;

  // Q as B-fragments pre-scaled by scale*log2(e).  The dO fragments are
  // re-read from L2 in every kv tile, inside the MFMA loop, although they
  // depend on the q row only: next to this kernel's 32 tr-read and 32
  // row-fragment address registers, keeping them resident spills (180 B
  // per lane against the 88 B it has now).  Each of those loads is
  // followed by a vmcnt(0) that also drains the staging DMAs of the next
  // tile; attn_bwd_dq_v3p_kernel below rebuilds the addresses and keeps
  // dO resident.  This kernel stays as the bit-reference (dq_variant 0).
  s16x8 q_b[8];
  float lse2, dvq;
#define DQ_LOAD_Q()                                                       \
  {                                                                       \
    const float qs = scale * 1.44269504088896340736f;                     \
    const unsigned short* src = Qb + (long long)my_q * q_rowstride;       \
    _Pragma("unroll") for (int ks = 0; ks < 8; ++ks) {                    \
      s16x8 raw = *(const s16x8*)(src + ks * 16 + h * 8);                 \
      _Pragma("unroll") for (int j = 0; j < 8; ++j)                       \
        raw[j] = (short)f2bf(bf2f((unsigned short)raw[j]) * qs);          \
      q_b[ks] = raw;                                                      \
    }                                                                     \
    float lv = lse[((long long)b * Hq + qh) * S + my_q];                  \
    lse2 = (lv == -INFINITY) ? 3.0e37f                                    \
                             : lv * 1.44269504088896340736f;              \
    dvq = Dvec[((long long)b * Hq + qh) * S + my_q];                      \
  }
  DQ_LOAD_Q();
  const unsigned short* do_src = dOb + (long long)my_q * q_rowstride;

  f32x16 dq_acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[dt][r] = 0.f;

  const int nt_A = causal ? (qbase + 128) / 64 : S / 64;
  const int nt_B = paired ? (qtB * 128 + 128) / 64 : 0;
  const int total_t = nt_A + nt_B;
  int w_tiles = causal ? ((qbase + 32 * w + 31) >> 6) + 1 : nt_A;

  // epilogue macro (runs at the pair boundary and at the end).
#define DQ_EPILOGUE()                                                     \
  {                                                                       \
    unsigned short* dQb = dQ + ((long long)b * S * Hq + qh) * ATT_D;      \
    unsigned short* qrow = dQb + (long long)my_q * q_rowstride;           \
    _Pragma("unroll") for (int dt = 0; dt < 4; ++dt)                      \
      _Pragma("unroll") for (int rq = 0; rq < 4; ++rq) {                  \
        s16x4 ov;                                                         \
        _Pragma("unroll") for (int r = 0; r < 4; ++r)                     \
          ov[r] = (short)f2bf(dq_acc[dt][rq * 4 + r] * scale);            \
        *(s16x4*)(qrow + dt * 32 + rq * 8 + h * 4) = ov;                  \
      }                                                                   \
  }

  // staging: wave w stages rows [16w,16w+16) of both K and V via 4+4
  // global_load_lds (linear dest, pre-swizzled source).
#define DQ_STAGE(kvoff, bufi)                                             \
  {                                                                       \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                       \
      int row = 16 * w + 4 * i + (lane >> 4);                             \
      int chunk = lane & 15;                                              \
      long long srcoff = (kvoff + row) * kv_rowstride;                    \
      int co = (chunk ^ (row & 15)) << 4;                                 \
      gload_lds16((const char*)(Kb + srcoff) + co,                        \
                  (char*)k_lds[bufi] + (16 * w + 4 * i) * 256);           \
      gload_lds16((const char*)(Vb + srcoff) + co,                        \
                  (char*)v_lds[bufi] + (16 * w + 4 * i) * 256);           \
    }                                                                     \
  }
  DQ_STAGE((long long)0, 0);

  for (int it = 0; it < total_t; ++it) {
    if (paired && it == nt_A) {
      DQ_EPILOGUE();
      qbase = qtB * 128;
      my_q = qbase + 32 * w + col;
      DQ_LOAD_Q();
      do_src = dOb + (long long)my_q * q_rowstride;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq_acc[dt][r] = 0.f;
      w_tiles = ((qbase + 32 * w + 31) >> 6) + 1;
    }
    const int kt = it < nt_A ? it : it - nt_A;
    const int buf = it & 1;
    vm_drain();  // hipcc's barrier wait is lgkm-only; drain the
                 // global_load_lds DMA for this buffer explicitly
    __syncthreads();
    if (it + 1 < total_t) {
      const int kt2 = (it + 1 < nt_A) ? it + 1 : it + 1 - nt_A;
      DQ_STAGE((long long)kt2 * 64, buf ^ 1);
    }
    if (kt >= w_tiles) continue;

    const int kvbase = kt * 64;
    // ---- S^T = K' Q^T and dP^T = V dO^T (4 interleaved chains).
    f32x16 st[2], dpt[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[n][r] = 0.f;
        dpt[n][r] = 0.f;
      }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        int krow = n * 32 + col;
        s16x8 akf = *(const s16x8*)(
            (char*)k_lds[buf] + swzK16(krow * 256 + (ks * 2 + h) * 16, krow));
        st[n] = MFMA32V3(as_bf16x8(akf), as_bf16x8(q_b[ks]), st[n]);
        s16x8 avf = *(const s16x8*)(
            (char*)v_lds[buf] + swzK16(krow * 256 + (ks * 2 + h) * 16, krow));
        s16x8 dof = *(const s16x8*)(do_src + ks * 16 + h * 8);
        dpt[n] = MFMA32V3(as_bf16x8(avf), as_bf16x8(dof), dpt[n]);
      }
    __builtin_amdgcn_s_setprio(0);

    // ---- P^T = exp2(S' - lse'); dS^T = P^T * (dP^T - Dvec[q]).
    if (causal && kvbase + 63 > qbase + 32 * w) {
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int kv = kvbase + n * 32 + (r & 3) + ((r >> 2) << 3) + (h << 2);
          if (kv > my_q) st[n][r] = -30000.f;
        }
    }
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float p = exp2f(st[n][r] - lse2);
        dpt[n][r] = p * (dpt[n][r] - dvq);
      }

    // ---- dQ^T += K^T dS^T: A = tr reads of the K tile (column
    // fragments over the swizzled layout), B = permlane pack of dS^T.
    tr4 t0, t1;
    s16x8 db;
#define DQ_TR_ISSUE(ks)                                                   \
  {                                                                       \
    unsigned base = (unsigned)(size_t)((char*)k_lds[buf]);                \
    int kv_s = (ks) * 16 + ((g >> 1) << 3) + (lw >> 2);                   \
    int d_s0 = ((g & 1) << 4) + ((lw & 3) << 2);                          \
    unsigned a0 = (unsigned)(kv_s * 256 +                                 \
                             ((((d_s0) >> 3) ^ (kv_s & 15)) << 4) +       \
                             ((d_s0 & 7) << 1));                          \
    unsigned a1 = (unsigned)((kv_s + 4) * 256 +                           \
                             ((((d_s0) >> 3) ^ ((kv_s + 4) & 15)) << 4) + \
                             ((d_s0 & 7) << 1));                          \
    unsigned a2 = (unsigned)(kv_s * 256 +                                 \
                             ((((32 + d_s0) >> 3) ^ (kv_s & 15)) << 4) +  \
                             ((d_s0 & 7) << 1));                          \
    unsigned a3 = (unsigned)((kv_s + 4) * 256 +                           \
                             ((((32 + d_s0) >> 3) ^ ((kv_s + 4) & 15))    \
                              << 4) +                                     \
                             ((d_s0 & 7) << 1));                          \
    ds_tr4_issue(&t0, base + a0, base + a1, base + a2, base + a3);        \
    unsigned a4 = (unsigned)(kv_s * 256 +                                 \
                             ((((64 + d_s0) >> 3) ^ (kv_s & 15)) << 4) +  \
                             ((d_s0 & 7) << 1));                          \
    unsigned a5 = (unsigned)((kv_s + 4) * 256 +                           \
                             ((((64 + d_s0) >> 3) ^ ((kv_s + 4) & 15))    \
                              << 4) +                                     \
                             ((d_s0 & 7) << 1));                          \
    unsigned a6 = (unsigned)(kv_s * 256 +                                 \
                             ((((96 + d_s0) >> 3) ^ (kv_s & 15)) << 4) +  \
                             ((d_s0 & 7) << 1));                          \
    unsigned a7 = (unsigned)((kv_s + 4) * 256 +                           \
                             ((((96 + d_s0) >> 3) ^ ((kv_s + 4) & 15))    \
                              << 4) +                                     \
                             ((d_s0 & 7) << 1));                          \
    ds_tr4_issue(&t1, base + a4, base + a5, base + a6, base + a7);        \
  }
#define DQ_MFMA(bfrag)                                                    \
  {                                                                       \
    union { unsigned long long u[2]; s16x8 v; } af;                       \
    __builtin_amdgcn_s_setprio(1);                                        \
    af.u[0] = t0.d[0];                                                    \
    af.u[1] = t0.d[1];                                                    \
    dq_acc[0] = MFMA32V3(as_bf16x8(af.v), as_bf16x8(bfrag), dq_acc[0]);   \
    af.u[0] = t0.d[2];                                                    \
    af.u[1] = t0.d[3];                                                    \
    dq_acc[1] = MFMA32V3(as_bf16x8(af.v), as_bf16x8(bfrag), dq_acc[1]);   \
    af.u[0] = t1.d[0];                                                    \
    af.u[1] = t1.d[1];                                                    \
    dq_acc[2] = MFMA32V3(as_bf16x8(af.v), as_bf16x8(bfrag), dq_acc[2]);   \
    af.u[0] = t1.d[2];                                                    \
    af.u[1] = t1.d[3];                                                    \
    dq_acc[3] = MFMA32V3(as_bf16x8(af.v), as_bf16x8(bfrag), dq_acc[3]);   \
    __builtin_amdgcn_s_setprio(0);                                        \
  }
    DQ_TR_ISSUE(0);
    V3_PACK2(db, dpt, 0);
    lgkm_wait0_bind2(&t0, &t1);
    DQ_MFMA(db);
    DQ_TR_ISSUE(1);
    V3_PACK2(db, dpt, 1);
    lgkm_wait0_bind2(&t0, &t1);
    DQ_MFMA(db);
    DQ_TR_ISSUE(2);
    V3_PACK2(db, dpt, 2);
    lgkm_wait0_bind2(&t0, &t1);
    DQ_MFMA(db);
    DQ_TR_ISSUE(3);
    V3_PACK2(db, dpt, 3);
    lgkm_wait0_bind2(&t0, &t1);
    DQ_MFMA(db);
  }

  DQ_EPILOGUE();
#undef DQ_EPILOGUE
#undef DQ_LOAD_Q
#undef DQ_STAGE
#undef DQ_TR_ISSUE
}

// ---------------------------------------------------------------------------
// Pipelined dq kernel: the grid, LDS tile layouts, MFMA sequence,
// accumulation order, exponent math and epilogue of attn_bwd_dq_v3_kernel
// (dQ is bit-identical); only the memory schedule and the register use
// differ.
//
//  * The lane's eight dO fragments depend on its q row only, so they are
//    loaded once per q tile next to Q/lse/Dvec and stay in 32 VGPRs.  The
//    tile loop then holds no ordinary global load, and its only vmcnt wait
//    is the vm_drain() in front of the handoff barrier: the staging DMAs
//    of tile t+1 stay in flight under all of tile t's MFMAs.
//  * The staging is unconditional (the block's last iteration restages its
//    own tile into the free buffer), so no wait has to cover a path
//    without it.
//  * One __shared__ array: the two K and two V buffers are compile-time
//    offsets of each other.  The 32 tr-read addresses are 8 lane bases
//    plus the DS offset field, the 32 row-fragment addresses one lane base
//    XOR (ks << 5) plus the offset field; the bases carry the buffer
//    parity and are flipped in place once per tile.
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256, 2) void attn_bwd_dq_v3p_kernel(
    const unsigned short* __restrict__ Q, const unsigned short* __restrict__ K,
    const unsigned short* __restrict__ V, const unsigned short* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ Dvec,
    unsigned short* __restrict__ dQ, int B, int S, int Hq, int Hkv,
    float scale, int causal) {
  // byte offsets: K buffer i at i * 16384, V buffer i at 32768 + i * 16384.
  __shared__ unsigned short lds[4 * 64 * ATT_D];

  const int nq = S / 128;
  const bool paired = causal && (int)gridDim.x * 2 == nq;
  const int qtA = paired ? nq - 1 - (int)blockIdx.x
                         : (int)gridDim.x - 1 - (int)blockIdx.x;
  const int qtB = paired ? (int)blockIdx.x : 0;
  const int bh = blockIdx.y;
  const int b = bh / Hq;
  const int qh = bh % Hq;
  const int kvh = qh / (Hq / Hkv);
  int qbase = qtA * 128;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int col = lane & 31;
  const int h = lane >> 5;
  const int g = lane >> 4;
  const int lw = lane & 15;

  const long long q_rowstride = (long long)Hq * ATT_D;
  const long long kv_rowstride = (long long)Hkv * ATT_D;
  const unsigned short* Qb = Q + ((long long)b * S * Hq + qh) * ATT_D;
  const unsigned short* Kb = K + ((long long)b * S * Hkv + kvh) * ATT_D;
  const unsigned short* Vb = V + ((long long)b * S * Hkv + kvh) * ATT_D;
  const unsigned short* dOb = dO + ((long long)b * S * Hq + qh) * ATT_D;
  const float* lse_b = lse + ((long long)b * Hq + qh) * S;
  const float* dvec_b = Dvec + ((long long)b * Hq + qh) * S;

  int my_q = qbase + 32 * w + col;

  // Q as B-fragments pre-scaled by scale*log2(e), and the dO B-fragments,
  // resident for the whole q tile.  The empty asm makes the dO registers
  // defined here, so their vmcnt wait sits here and not in the tile loop.
  s16x8 q_b[8], do_b[8];
  float lse2, dvq;
#define DQP_LOAD_Q()                                                      \
  {                                                                       \
    const float qs = scale * 1.44269504088896340736f;                     \
    const unsigned short* src = Qb + (long long)my_q * q_rowstride;       \
    const unsigned short* dsrc = dOb + (long long)my_q * q_rowstride;     \
    _Pragma("unroll") for (int ks = 0; ks < 8; ++ks)                      \
      do_b[ks] = *(const s16x8*)(dsrc + ks * 16 + h * 8);                 \
    _Pragma("unroll") for (int ks = 0; ks < 8; ++ks) {                    \
      s16x8 raw = *(const s16x8*)(src + ks * 16 + h * 8);                 \
      _Pragma("unroll") for (int j = 0; j < 8; ++j)                       \
        raw[j] = (short)f2bf(bf2f((unsigned short)raw[j]) * qs);          \
      q_b[ks] = raw;                                                      \
    }                                                                     \
    float lv = lse_b[my_q];                                               \
    lse2 = (lv == -INFINITY) ? 3.0e37f                                    \
                             : lv * 1.44269504088896340736f;              \
    dvq = dvec_b[my_q];                                                   \
    _Pragma("unroll") for (int ks = 0; ks < 8; ++ks)                      \
      asm volatile("" : "+v"(do_b[ks]));                                  \
    asm volatile("" : "+v"(lse2), "+v"(dvq));                             \
  }

  f32x16 dq_acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[dt][r] = 0.f;

  const int nt_A = causal ? (qbase + 128) / 64 : S / 64;
  const int nt_B = paired ? (qtB * 128 + 128) / 64 : 0;
  const int total_t = nt_A + nt_B;
  int w_tiles = causal ? ((qbase + 32 * w + 31) >> 6) + 1 : nt_A;

#define DQP_EPILOGUE()                                                    \
  {                                                                       \
    unsigned short* dQb = dQ + ((long long)b * S * Hq + qh) * ATT_D;      \
    unsigned short* qrow = dQb + (long long)my_q * q_rowstride;           \
    _Pragma("unroll") for (int dt = 0; dt < 4; ++dt)                      \
      _Pragma("unroll") for (int rq = 0; rq < 4; ++rq) {                  \
        s16x4 ov;                                                         \
        _Pragma("unroll") for (int r = 0; r < 4; ++r)                     \
          ov[r] = (short)f2bf(dq_acc[dt][rq * 4 + r] * scale);            \
        *(s16x4*)(qrow + dt * 32 + rq * 8 + h * 4) = ov;                  \
      }                                                                   \
  }

  // Staging: wave w stages rows [16w, 16w+16) of both K and V via 4 + 4
  // global_load_lds (linear dest, pre-swizzled source) from a wave-uniform
  // tile base plus a 32-bit lane offset.  Row 16w + 4i + g of the tile,
  // chunk lw ^ (4i + g): i moves the row by 4 and flips chunk bits 2..3.
  const unsigned kv_rs2 = (unsigned)kv_rowstride * 2u;  // row stride, bytes
  const unsigned sg_off =
      (unsigned)(16 * w + g) * kv_rs2 + (unsigned)((lw ^ g) << 4);
#define DQP_STAGE(kvrow0, bufi)                                           \
  {                                                                       \
    gptr_t ksrc = uniform_ptr(Kb + (long long)(kvrow0) * kv_rowstride);   \
    gptr_t vsrc = uniform_ptr(Vb + (long long)(kvrow0) * kv_rowstride);   \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                       \
      const unsigned off = (sg_off ^ (unsigned)(i << 6)) + 4u * i * kv_rs2; \
      char* dst = (char*)lds + (bufi) * 16384 + (16 * w + 4 * i) * 256;   \
      gload_lds16(ksrc + off, dst);                                       \
      gload_lds16(vsrc + off, dst + 32768);                               \
    }                                                                     \
  }

  // Lane bases inside the K buffer, initialised for buffer 1 and flipped
  // at the top of every tile (so tile 0 reads buffer 0).
  //  * tra: the eight tr-read addresses of k-step 0; k-step ks moves kv_s
  //    by 16 rows = +4096 B and leaves the swizzle key kv_s & 15 alone.
  //  * frag: swzK16(col*256 + h*16, col), the row-fragment address of
  //    k-step 0 for n = 0; k-step ks is ^ (ks << 5), n = 1 is +8192 (the
  //    key (32 + col) & 15 is the same) and V is +32768.
  unsigned tra[8];
  {
    const int kv_s = ((g >> 1) << 3) + (lw >> 2);
    const int d_s0 = ((g & 1) << 4) + ((lw & 3) << 2);
    const unsigned base = (unsigned)(size_t)((char*)lds) + 16384u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int kv = kv_s + 4 * (i & 1);
      const int d = 32 * (i >> 1) + d_s0;
      tra[i] = base + (unsigned)(kv * 256 + (((d >> 3) ^ (kv & 15)) << 4) +
                                 ((d & 7) << 1));
    }
  }
  unsigned frag = (unsigned)swzK16(col * 256 + h * 16, col) + 16384u;

  DQP_LOAD_Q();
  DQP_STAGE(0, 0);

  for (int it = 0; it < total_t; ++it) {
    if (paired && it == nt_A) {
      DQP_EPILOGUE();
      qbase = qtB * 128;
      my_q = qbase + 32 * w + col;
      DQP_LOAD_Q();
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq_acc[dt][r] = 0.f;
      w_tiles = ((qbase + 32 * w + 31) >> 6) + 1;
    }
    const int kt = it < nt_A ? it : it - nt_A;
    const int buf = it & 1;
    {
      const unsigned flip = buf ? 16384u : (unsigned)-16384;
      frag += flip;
#pragma unroll
      for (int i = 0; i < 8; ++i) tra[i] += flip;
    }
    vm_drain();  // the only vmcnt wait of the loop: the DMA of this
                 // buffer, issued a whole tile ago
    __syncthreads();
    {
      // next tile, or on the block's last iteration this tile again (a
      // row range already read, into the free buffer).
      const int nx = it + 1 < total_t ? it + 1 : it;
      const int kt2 = nx < nt_A ? nx : nx - nt_A;
      DQP_STAGE(kt2 * 64, buf ^ 1);
    }
    if (kt >= w_tiles) continue;

    const int kvbase = kt * 64;
    // ---- S^T = K' Q^T and dP^T = V dO^T (4 interleaved chains).
    f32x16 st[2], dpt[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[n][r] = 0.f;
        dpt[n][r] = 0.f;
      }
    // The fragment address is rebuilt per k-step by one XOR; the empty
    // asm keeps the eight results from being hoisted into registers.
    unsigned fr = frag;
    asm volatile("" : "+v"(fr));
    // MFMA i = 4 ks + 2 n + (0: S chain, 1: dP chain) takes fragment i
    // (K or V rows n*32 + col, k-step ks).  The reads are split-phase
    // like the tr reads: four fragments (the two K/V pairs of one k-step)
    // are in flight ahead of the MFMA that consumes them, each MFMA is
    // followed by the read of the fragment four later into the registers
    // it has just consumed, and every wait is a counted lgkmcnt(3).
    // (With plain C++ loads hipcc waits lgkmcnt(0) here: while a
    // global_load_lds is outstanding it treats the LGKM counter as
    // unordered.)
    s16x8 fa[4];
#define DQP_RD(i)                                                         \
  ds_read128_issue_off<(((i) >> 1) & 1) * 8192 + ((i) & 1) * 32768>(      \
      &fa[(i) & 3], fr ^ (unsigned)(((i) >> 2) << 5))
#define DQP_STEP(i)                                                       \
  {                                                                       \
    lgkm_wait_bind1<((i) < 28 ? 3 : 31 - (i))>(&fa[(i) & 3]);             \
    if ((i) & 1)                                                          \
      dpt[((i) >> 1) & 1] =                                               \
          MFMA32V3(as_bf16x8(fa[(i) & 3]), as_bf16x8(do_b[(i) >> 2]),     \
                   dpt[((i) >> 1) & 1]);                                  \
    else                                                                  \
      st[((i) >> 1) & 1] =                                                \
          MFMA32V3(as_bf16x8(fa[(i) & 3]), as_bf16x8(q_b[(i) >> 2]),      \
                   st[((i) >> 1) & 1]);                                   \
    __builtin_amdgcn_sched_barrier(0);                                    \
    if ((i) + 4 < 32) DQP_RD((i) + 4);                                    \
  }
#define DQP_STEP4(i)                                                      \
  DQP_STEP(i) DQP_STEP((i) + 1) DQP_STEP((i) + 2) DQP_STEP((i) + 3)
    __builtin_amdgcn_s_setprio(1);
    DQP_RD(0);
    DQP_RD(1);
    DQP_RD(2);
    DQP_RD(3);
    DQP_STEP4(0) DQP_STEP4(4) DQP_STEP4(8) DQP_STEP4(12)
    DQP_STEP4(16) DQP_STEP4(20) DQP_STEP4(24) DQP_STEP4(28)
    __builtin_amdgcn_s_setprio(0);
#undef DQP_STEP4
#undef DQP_STEP
#undef DQP_RD

    // ---- P^T = exp2(S' - lse'); dS^T = P^T * (dP^T - Dvec[q]).
    if (causal && kvbase + 63 > qbase + 32 * w) {
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int kv = kvbase + n * 32 + (r & 3) + ((r >> 2) << 3) + (h << 2);
          if (kv > my_q) st[n][r] = -30000.f;
        }
    }
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float p = exp2f(st[n][r] - lse2);
        dpt[n][r] = p * (dpt[n][r] - dvq);
      }

    // ---- dQ^T += K^T dS^T: A = tr reads of the K tile (column
    // fragments over the swizzled layout), B = permlane pack of dS^T.
    tr4 t0, t1;
    s16x8 db;
#define DQP_TR_ISSUE(ks)                                                  \
  {                                                                       \
    ds_tr4_issue_off_ec<(ks) * 4096>(&t0, tra[0], tra[1], tra[2], tra[3]); \
    ds_tr4_issue_off_ec<(ks) * 4096>(&t1, tra[4], tra[5], tra[6], tra[7]); \
  }
    DQP_TR_ISSUE(0);
    V3_PACK2(db, dpt, 0);
    lgkm_wait0_bind2(&t0, &t1);
    DQ_MFMA(db);
    DQP_TR_ISSUE(1);
    V3_PACK2(db, dpt, 1);
    lgkm_wait0_bind2(&t0, &t1);
    DQ_MFMA(db);
    DQP_TR_ISSUE(2);
    V3_PACK2(db, dpt, 2);
    lgkm_wait0_bind2(&t0, &t1);
    DQ_MFMA(db);
    DQP_TR_ISSUE(3);
    V3_PACK2(db, dpt, 3);
    lgkm_wait0_bind2(&t0, &t1);
    DQ_MFMA(db);
  }
  // The last iteration's restaging is still in flight: it must land
  // before the block gives its LDS back.
  vm_drain();

  DQP_EPILOGUE();
#undef DQP_EPILOGUE
#undef DQP_LOAD_Q
#undef DQP_STAGE
#undef DQP_TR_ISSUE
#undef DQ_MFMA
}

// dkv_variant: 0 = attn_bwd_dkv_v3_kernel, 1 = the pipelined kernel,
// 2 = the pipelined kernel on the heavy-first grid; -1 = 2, the shipped
// choice.  Measured per call at B6 S4096 Hq32 Hkv8 causal: 4.13 / 3.62 /
// 2.14 ms (docs/BENCHMARKS.md).
extern "C" void attn_bwd_v3_launch(const void* Q, const void* K,
                                   const void* V, const void* dO,
                                   const float* lse, const float* Dvec,
                                   void* dQ, void* dK, void* dV, int B,
                                   int S, int Hq, int Hkv, float scale,
                                   bool causal, int dkv_variant,
                                   int dq_variant, hipStream_t stream) {
  const int variant = dkv_variant >= 0 ? dkv_variant : 2;
  if (variant == 0) {
    dim3 gkv(S / 128, B * Hkv);
    hipLaunchKernelGGL(attn_bwd_dkv_v3_kernel, gkv, dim3(256), 0, stream,
                       (const unsigned short*)Q, (const unsigned short*)K,
                       (const unsigned short*)V, (const unsigned short*)dO,
                       lse, Dvec, (unsigned short*)dK, (unsigned short*)dV,
                       B, S, Hq, Hkv, scale, causal ? 1 : 0);
  } else {
    // heavy-first: x (fastest dispatched) runs over (b, kv-head), y over
    // the kv tile, so all kt = 0 blocks start before any kt = 1 block.
    const int heavy_first = variant == 2 ? 1 : 0;
    dim3 gkv = heavy_first ? dim3(B * Hkv, S / 128) : dim3(S / 128, B * Hkv);
    hipLaunchKernelGGL(attn_bwd_dkv_v3p_kernel, gkv, dim3(256), 0, stream,
                       (const unsigned short*)Q, (const unsigned short*)K,
                       (const unsigned short*)V, (const unsigned short*)dO,
                       lse, Dvec, (unsigned short*)dK, (unsigned short*)dV,
                       B, S, Hq, Hkv, scale, causal ? 1 : 0, heavy_first);
  }
  int nqq = S / 128;
  int gqx = (causal && nqq % 2 == 0) ? nqq / 2 : nqq;
  dim3 gq(gqx, B * Hq);
  // dq_variant: 0 = attn_bwd_dq_v3_kernel, 1 = the pipelined kernel;
  // -1 = 1, the shipped choice.  Measured per call at B6 S4096 Hq32 Hkv8
  // causal: 2.25 / 1.31 ms, dQ bit-identical (docs/BENCHMARKS.md).
  const int dqv = dq_variant >= 0 ? dq_variant : 1;
  hipLaunchKernelGGL(dqv == 1 ? attn_bwd_dq_v3p_kernel : attn_bwd_dq_v3_kernel,
                     gq, dim3(256), 0, stream,
                     (const unsigned short*)Q, (const unsigned short*)K,
                     (const unsigned short*)V, (const unsigned short*)dO,
                     lse, Dvec, (unsigned short*)dQ, B, S, Hq, Hkv, scale,
                     causal ? 1 : 0);
}
