// Flash-attention backward (causal, GQA, D=128, bf16) for CDNA4/gfx950.
//
// Three kernels, no atomics (FA2-style split):
//   1. attn_bwd_pre:  Dvec = rowsum(dO * O)               [B,Hq,S] fp32
//   2. attn_bwd_dkv:  one block per kv tile; loops grouped q-heads and
//      q tiles >= diagonal; accumulates dK, dV in registers.
//   3. attn_bwd_dq:   one block per q tile; loops kv tiles <= diagonal.
// The 64-tile dkv/dq kernels stage swizzled LDS tiles per iteration
// (normal + transposed copies where the contraction axis demands it);
// the v3 dkv/dq kernels that S % 128 == 0 runs are in
// attention_bwd_v3.hip.  The dispatch is at the end of this file.
//
// Math (P normalized via saved lse): P = exp(scale*QK^T - lse);
// dV = P^T dO; dP = dO V^T; dS = P*(dP - Dvec); dQ = scale*dS*K;
// dK = scale*dS^T*Q.
#include "attn_launch.h"
#include "common.h"

#define BM 64
#define BN 64

// ---------------------------------------------------------------------------
// Dvec preprocess: one wave per (b, qh, s) row.
// ---------------------------------------------------------------------------
extern "C" __global__ void attn_bwd_pre_kernel(
    const unsigned short* __restrict__ dO, const unsigned short* __restrict__ O,
    float* __restrict__ Dvec, long long rows, int S, int Hq) {
  const int lane = threadIdx.x & 63;
  const long long wave_id =
      (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long long stride = (long long)gridDim.x * (blockDim.x >> 6);
  for (long long row = wave_id; row < rows; row += stride) {
    // row = (b*S + s)*Hq + h ; layout [B,S,Hq,D] is contiguous in rows*D,
    // so consecutive waves keep reading consecutive 256 B rows.
    const unsigned short* drow = dO + row * ATT_D;
    const unsigned short* orow = O + row * ATT_D;
    float acc = bf2f(drow[lane]) * bf2f(orow[lane]) +
                bf2f(drow[lane + 64]) * bf2f(orow[lane + 64]);
    acc = wave_reduce_sum(acc);
    // Dvec is stored [B,Hq,S], the layout lse has: contiguous in s, so
    // the dkv/dq kernels read a lane's runs of q rows as float4.
    const int hh = (int)(row % Hq);
    const long long bs = row / Hq;
    const int ss = (int)(bs % S);
    const long long bb = bs / S;
    if (lane == 0) Dvec[(bb * Hq + hh) * S + ss] = acc;
  }
}

// ---------------------------------------------------------------------------
// dK/dV kernel. Grid: (S/BN, B*Hkv). LDS: Q,QT,dO,dOT (16KB each) + 8KB
// shared P/dS staging = 72KB -> 2 blocks/CU.
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256, 2) void attn_bwd_dkv_kernel(
    const unsigned short* __restrict__ Q, const unsigned short* __restrict__ K,
    const unsigned short* __restrict__ V, const unsigned short* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ Dvec,
    unsigned short* __restrict__ dK, unsigned short* __restrict__ dV, int B,
    int S, int Hq, int Hkv, float scale, int causal) {
  __shared__ unsigned short q_lds[BM * ATT_D];
  __shared__ unsigned short qt_lds[ATT_D * BM];
  __shared__ unsigned short do_lds[BM * ATT_D];
  __shared__ unsigned short dot_lds[ATT_D * BM];
  __shared__ unsigned short p_lds[BN * BM];   // PT
  __shared__ unsigned short ds_lds[BN * BM];  // dST (separate so both
                                              // mfma passes share 1 barrier)

  const int kt = blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / Hkv;
  const int kvh = bh % Hkv;
  const int group = Hq / Hkv;
  const int kvbase = kt * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;    // wave owns kv rows [16w, 16w+16)
  const int lrow = lane & 15;
  const int lgrp = lane >> 4;

  const long long q_rowstride = (long long)Hq * ATT_D;
  const long long kv_rowstride = (long long)Hkv * ATT_D;
  const unsigned short* Kb = K + ((long long)b * S * Hkv + kvh) * ATT_D;
  const unsigned short* Vb = V + ((long long)b * S * Hkv + kvh) * ATT_D;

  // K,V fragments for this wave's 16 kv rows (A-operand, fixed).
  s16x8 a_k[4], a_v[4];
  {
    const int kvrow = kvbase + 16 * w + lrow;
    const unsigned short* ksrc = Kb + (long long)kvrow * kv_rowstride;
    const unsigned short* vsrc = Vb + (long long)kvrow * kv_rowstride;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      a_k[ks] = *(const s16x8*)(ksrc + ks * 32 + lgrp * 8);
      a_v[ks] = *(const s16x8*)(vsrc + ks * 32 + lgrp * 8);
    }
  }

  f32x4 dv_acc[8], dk_acc[8];
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) {
    dv_acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    dk_acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  for (int g = 0; g < group; ++g) {
    const int qh = kvh * group + g;
    const unsigned short* Qb = Q + ((long long)b * S * Hq + qh) * ATT_D;
    const unsigned short* dOb = dO + ((long long)b * S * Hq + qh) * ATT_D;
    const float* lse_b = lse + ((long long)b * Hq + qh) * S;
    // Dvec stored [B,Hq,S] like lse (see pre kernel).
    const float* dvec_b = Dvec + ((long long)b * Hq + qh) * S;

    const int qt0 = causal ? kvbase / BM : 0;
    for (int qt = qt0; qt < S / BM; ++qt) {
      const int qbase = qt * BM;
      __syncthreads();
      // Stage Q, QT, dO, dOT (swizzled).
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // 8-row x 8-chunk staging map: scatter writes hit all 32 banks
        // (see the staging comment in attention_fwd.hip).
        int ch = (tid & 7) | ((i & 1) << 3);
        int row = (tid >> 3) | ((i >> 1) << 5);
        s16x8 qv = *(const s16x8*)(Qb + (long long)(qbase + row) * q_rowstride + ch * 8);
        *(s16x8*)((char*)q_lds + swz(row * 256 + ch * 16, row)) = qv;
        s16x8 dov = *(const s16x8*)(dOb + (long long)(qbase + row) * q_rowstride + ch * 8);
        *(s16x8*)((char*)do_lds + swz(row * 256 + ch * 16, row)) = dov;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int d = ch * 8 + j;
          *(unsigned short*)((char*)qt_lds + swzT(d * 128 + row * 2, d)) =
              (unsigned short)qv[j];
          *(unsigned short*)((char*)dot_lds + swzT(d * 128 + row * 2, d)) =
              (unsigned short)dov[j];
        }
      }
      __syncthreads();

      // ST = K Q^T (raw);  [kv 16][q 64] per wave.
      f32x4 st[4], dpt[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        st[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        dpt[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          int qrow = ct * 16 + lrow;
          s16x8 bq = *(const s16x8*)((char*)q_lds +
                                     swz(qrow * 256 + (ks * 32 + lgrp * 8) * 2, qrow));
          st[ct] = MFMA_BF16(as_bf16x8(a_k[ks]), as_bf16x8(bq), st[ct]);
          s16x8 bdo = *(const s16x8*)((char*)do_lds +
                                      swz(qrow * 256 + (ks * 32 + lgrp * 8) * 2, qrow));
          dpt[ct] = MFMA_BF16(as_bf16x8(a_v[ks]), as_bf16x8(bdo), dpt[ct]);
        }
      }

      // PT = exp(scale*ST - lse[q]); dST = PT * (dPT - Dvec[q]).
      // Streamed straight to LDS (no pt/dst register arrays — keeping
      // them cost 32 VGPRs and dropped occupancy to 1 wave/SIMD).
      const int my_kvrow = kvbase + 16 * w + lgrp * 4;  // + r
      // No barrier needed before the P/dS writes: the prior iteration's
      // dV/dK reads of these buffers completed before this iteration's
      // top-of-loop barrier (two barriers ago).
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        int qcol = qbase + ct * 16 + lrow;
        float l = lse_b[qcol];
        float dv = dvec_b[qcol];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float sv = st[ct][r] * scale;
          float pv;
          if ((causal && qcol < my_kvrow + r) || l == -INFINITY)
            pv = 0.f;
          else
            pv = __expf(sv - l);
          int prow = 16 * w + lgrp * 4 + r;
          int pcol = ct * 16 + lrow;
          int off = swzP(prow * 128 + pcol * 2, prow);
          *(unsigned short*)((char*)p_lds + off) = f2bf(pv);
          *(unsigned short*)((char*)ds_lds + off) =
              f2bf(pv * (dpt[ct][r] - dv));
        }
      }
      __syncthreads();

      // dV += PT * dO (via dOT);  dK += dST * Q (via QT).
#pragma unroll
      for (int ct = 0; ct < 8; ++ct)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          int prow = 16 * w + lrow;
          int a_off = swzP(prow * 128 + (ks * 32 + lgrp * 8) * 2, prow);
          int brow = ct * 16 + lrow;
          int b_off = swzT(brow * 128 + (ks * 32 + lgrp * 8) * 2, brow);
          s16x8 pfrag = *(const s16x8*)((char*)p_lds + a_off);
          s16x8 dofrag = *(const s16x8*)((char*)dot_lds + b_off);
          dv_acc[ct] = MFMA_BF16(as_bf16x8(pfrag), as_bf16x8(dofrag),
                                 dv_acc[ct]);
          s16x8 dsfrag = *(const s16x8*)((char*)ds_lds + a_off);
          s16x8 qfrag = *(const s16x8*)((char*)qt_lds + b_off);
          dk_acc[ct] = MFMA_BF16(as_bf16x8(dsfrag), as_bf16x8(qfrag),
                                 dk_acc[ct]);
        }
    }
  }

  // Write dK, dV (bf16), applying scale to dK.
  unsigned short* dKb = dK + ((long long)b * S * Hkv + kvh) * ATT_D;
  unsigned short* dVb = dV + ((long long)b * S * Hkv + kvh) * ATT_D;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kvrow = kvbase + 16 * w + lgrp * 4 + r;
    unsigned short* krow = dKb + (long long)kvrow * kv_rowstride;
    unsigned short* vrow = dVb + (long long)kvrow * kv_rowstride;
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) {
      krow[ct * 16 + lrow] = f2bf(dk_acc[ct][r] * scale);
      vrow[ct * 16 + lrow] = f2bf(dv_acc[ct][r]);
    }
  }
}

// ---------------------------------------------------------------------------
// Swapped-operand dQ kernel (same trick as attn_fwd_swapped_kernel):
// S^T = K Q^T and dP^T = V dO^T put q on lanes, so P^T/dS^T stay in
// registers (lse/Dvec become per-lane scalars) and dQ^T = K^T dS^T
// consumes dS^T as shuffled B-fragments — the ds_lds roundtrip and one
// of the two barriers per tile disappear.
// ---------------------------------------------------------------------------
// (launch_bounds(256,3) forces 168 VGPRs + 100 B/lane scratch for 3
// waves/SIMD: measured 158 vs 169 TF/s — spills cost more than the
// extra wave hides.)
extern "C" __global__ __launch_bounds__(256, 1) void attn_bwd_dq_swapped_kernel(
    const unsigned short* __restrict__ Q, const unsigned short* __restrict__ K,
    const unsigned short* __restrict__ V, const unsigned short* __restrict__ dO,
    const float* __restrict__ lse, const float* __restrict__ Dvec,
    unsigned short* __restrict__ dQ, int B, int S, int Hq, int Hkv,
    float scale, int causal) {
  __shared__ unsigned short k_lds[BN * ATT_D];
  __shared__ unsigned short kt_lds[ATT_D * BN];
  __shared__ unsigned short v_lds[BN * ATT_D];

  const int qt = gridDim.x - 1 - blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / Hq;
  const int qh = bh % Hq;
  const int kvh = qh / (Hq / Hkv);
  const int qbase = qt * BM;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int lrow = lane & 15;
  const int lgrp = lane >> 4;

  const long long q_rowstride = (long long)Hq * ATT_D;
  const long long kv_rowstride = (long long)Hkv * ATT_D;
  const unsigned short* Qb = Q + ((long long)b * S * Hq + qh) * ATT_D;
  const unsigned short* Kb = K + ((long long)b * S * Hkv + kvh) * ATT_D;
  const unsigned short* Vb = V + ((long long)b * S * Hkv + kvh) * ATT_D;
  const unsigned short* dOb = dO + ((long long)b * S * Hq + qh) * ATT_D;
  const float* lse_b = lse + ((long long)b * Hq + qh) * S;
  const float* dvec_b = Dvec + ((long long)b * Hq + qh) * S;

  // Q / dO as B-fragments (the same bytes A-fragment loads would
  // fetch); lse/D collapse to per-lane scalars.
  s16x8 q_b[4], do_b[4];
  const int my_q = qbase + 16 * w + lrow;
  {
    const unsigned short* qsrc = Qb + (long long)my_q * q_rowstride;
    const unsigned short* dsrc = dOb + (long long)my_q * q_rowstride;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      q_b[ks] = *(const s16x8*)(qsrc + ks * 32 + lgrp * 8);
      do_b[ks] = *(const s16x8*)(dsrc + ks * 32 + lgrp * 8);
    }
  }
  const float my_lse = lse_b[my_q];
  const float my_dvec = dvec_b[my_q];

  f32x4 dq_t[8];  // dQ^T: C[row=d=ct*16+lgrp*4+r][col=q=lrow]
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) dq_t[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int n_kv_tiles = causal ? (qbase + BM + BN - 1) / BN : S / BN;
  for (int kt = 0; kt < n_kv_tiles; ++kt) {
    const int kvbase = kt * BN;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int ch = (tid & 7) | ((i & 1) << 3);
      int row = (tid >> 3) | ((i >> 1) << 5);
      s16x8 kv8 = *(const s16x8*)(Kb + (long long)(kvbase + row) * kv_rowstride + ch * 8);
      *(s16x8*)((char*)k_lds + swz(row * 256 + ch * 16, row)) = kv8;
      s16x8 vv8 = *(const s16x8*)(Vb + (long long)(kvbase + row) * kv_rowstride + ch * 8);
      *(s16x8*)((char*)v_lds + swz(row * 256 + ch * 16, row)) = vv8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int d = ch * 8 + j;
        *(unsigned short*)((char*)kt_lds + swzT(d * 128 + row * 2, d)) =
            (unsigned short)kv8[j];
      }
    }
    __syncthreads();

    // S^T = K Q^T, dP^T = V dO^T (interleaved independent chains).
    f32x4 st[4], dpt[4];
#pragma unroll
    for (int kv4 = 0; kv4 < 4; ++kv4) {
      st[kv4] = f32x4{0.f, 0.f, 0.f, 0.f};
      dpt[kv4] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int kv4 = 0; kv4 < 4; ++kv4) {
        int krow = kv4 * 16 + lrow;
        s16x8 a_k = *(const s16x8*)((char*)k_lds +
            swz(krow * 256 + (ks * 32 + lgrp * 8) * 2, krow));
        st[kv4] = MFMA_BF16(as_bf16x8(a_k), as_bf16x8(q_b[ks]), st[kv4]);
        s16x8 a_v = *(const s16x8*)((char*)v_lds +
            swz(krow * 256 + (ks * 32 + lgrp * 8) * 2, krow));
        dpt[kv4] = MFMA_BF16(as_bf16x8(a_v), as_bf16x8(do_b[ks]),
                             dpt[kv4]);
      }

    // dS^T = P^T * (dP^T - D);  P^T = exp(scale*S^T - lse).
#pragma unroll
    for (int kv4 = 0; kv4 < 4; ++kv4)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int kv = kvbase + kv4 * 16 + lgrp * 4 + r;
        float pv;
        if ((causal && kv > my_q) || my_lse == -INFINITY)
          pv = 0.f;
        else
          pv = __expf(st[kv4][r] * scale - my_lse);
        st[kv4][r] = pv * (dpt[kv4][r] - my_dvec);
      }

    // dS^T -> B-fragments (same shuffle recipe as attn_fwd_swapped).
    s16x8 ds_b[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int src = (2 * (lgrp & 1) + (j >> 2)) * 16 + lrow;
        float v0 = __shfl(st[2 * ks][j & 3], src, 64);
        float v1 = __shfl(st[2 * ks + 1][j & 3], src, 64);
        ds_b[ks][j] = (short)f2bf((lgrp >> 1) ? v1 : v0);
      }

    // dQ^T += K^T dS^T : A from kt_lds.
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        int krow = ct * 16 + lrow;
        s16x8 a_kt = *(const s16x8*)((char*)kt_lds +
            swzT(krow * 128 + (ks * 32 + lgrp * 8) * 2, krow));
        dq_t[ct] = MFMA_BF16(as_bf16x8(a_kt), as_bf16x8(ds_b[ks]),
                             dq_t[ct]);
      }
  }

  unsigned short* dQb = dQ + ((long long)b * S * Hq + qh) * ATT_D;
  unsigned short* orow = dQb + (long long)my_q * q_rowstride;
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) {
    s16x4 ov;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      ov[r] = (short)f2bf(dq_t[ct][r] * scale);
    *(s16x4*)(orow + ct * 16 + lgrp * 4) = ov;
  }
}

// Backward dispatch: the Dvec preprocess always runs; then S % 128 == 0
// runs the v3 dkv/dq kernels (dkv_variant and dq_variant pick among them,
// see attn_bwd_v3_launch) and every other S % 64 == 0 runs the 64-tile
// kernels above.  They stay because they are the only path for the
// shapes v3 does not take, such as a sequence padded to 64 rows.
extern "C" void attn_bwd_launch(const void* Q, const void* K, const void* V,
                                const void* O, const void* dO,
                                const float* lse, float* Dvec, void* dQ,
                                void* dK, void* dV, int B, int S, int Hq,
                                int Hkv, float scale, bool causal,
                                int dkv_variant, int dq_variant,
                                hipStream_t stream) {
  long long rows = (long long)B * S * Hq;
  hipLaunchKernelGGL(attn_bwd_pre_kernel, dim3(membound_grid(rows, 4)),
                     dim3(256), 0, stream, (const unsigned short*)dO,
                     (const unsigned short*)O, Dvec, rows, S, Hq);
  if (S % 128 == 0) {
    attn_bwd_v3_launch(Q, K, V, dO, lse, Dvec, dQ, dK, dV, B, S, Hq, Hkv,
                       scale, causal, dkv_variant, dq_variant, stream);
    return;
  }
  hipLaunchKernelGGL(attn_bwd_dkv_kernel, dim3(S / BN, B * Hkv), dim3(256),
                     0, stream, (const unsigned short*)Q,
                     (const unsigned short*)K, (const unsigned short*)V,
                     (const unsigned short*)dO, lse, Dvec,
                     (unsigned short*)dK, (unsigned short*)dV, B, S, Hq, Hkv,
                     scale, causal ? 1 : 0);
  hipLaunchKernelGGL(attn_bwd_dq_swapped_kernel, dim3(S / BM, B * Hq),
                     dim3(256), 0, stream, (const unsigned short*)Q,
                     (const unsigned short*)K, (const unsigned short*)V,
                     (const unsigned short*)dO, lse, Dvec,
                     (unsigned short*)dQ, B, S, Hq, Hkv, scale,
                     causal ? 1 : 0);
}

