// Body of the append-attention kernel (attention_append.hip), included
// once per K/V source so that each instantiation is a kernel of its own
// with its pointer arguments __restrict__ at kernel level (as a function
// template inlined into two wrappers the bf16 kernel took 240 VGPRs
// instead of 218).  The includer defines
//   APPEND_KERNEL  the extern "C" kernel name,
//   APPEND_FP8     0: bf16 cache, append_load_tile into kpre/vpre;
//                  1: FP8 KV cache, AppendTileFp8, and the kernel takes
//                     the exponent tensors Ke, Ve.
// No include guard: this file is meant to be included more than once.
#if APPEND_FP8
#define APPEND_ELEM unsigned char
#define APPEND_LOAD(base) tile.load(base, kv_len, tid)
#define APPEND_K(i) tile.k(i)
#define APPEND_V(i) tile.v(i)
#else
#define APPEND_ELEM unsigned short
#define APPEND_LOAD(base) \
  append_load_tile(Kb, Vb, kv_rowstride, base, kv_len, tid, kpre, vpre)
#define APPEND_K(i) kpre[i]
#define APPEND_V(i) vpre[i]
#endif
extern "C" __global__ __launch_bounds__(256, 2) void APPEND_KERNEL(
    const unsigned short* __restrict__ Q,
    const APPEND_ELEM* __restrict__ Kc,
    const APPEND_ELEM* __restrict__ Vc,
#if APPEND_FP8
    const unsigned char* __restrict__ Ke,
    const unsigned char* __restrict__ Ve,
#endif
    unsigned short* __restrict__ O, const int* __restrict__ slot_ids,
    const int* __restrict__ q_start, const int* __restrict__ q_lens, int Sq,
    int Hq, int Hkv, int slots, int S_max, float scale) {
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

#if APPEND_FP8
  AppendTileFp8 tile(Kc, Vc, Ke, Ve, (long long)slot * S_max * Hkv + kvh,
                     kv_rowstride, Hkv);
#else
  const unsigned short* Kb =
      Kc + ((long long)slot * S_max * Hkv + kvh) * ATT_D;
  const unsigned short* Vb =
      Vc + ((long long)slot * S_max * Hkv + kvh) * ATT_D;
  s16x8 kpre[4], vpre[4];
#endif

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

  APPEND_LOAD(0);

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
          APPEND_K(i);
      const s16x8 vrow8 = APPEND_V(i);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int d = s_ch * 8 + j;
        *(unsigned short*)((char*)vt_lds + swzT(d * 128 + s_row * 2, d)) =
            (unsigned short)vrow8[j];
      }
    }
    __syncthreads();
    if (kt + 1 < n_kv_tiles)
      APPEND_LOAD((kt + 1) * BN);
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
        p_b[ks][j] = (short)f2bf((lgrp >> 1) ? v1 : v0);
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
#undef APPEND_ELEM
#undef APPEND_LOAD
#undef APPEND_K
#undef APPEND_V
