// Body of the grouped split-KV decode kernel (attention_decode_gqa.hip),
// included once per K/V source so that each instantiation is a kernel of
// its own with its pointer arguments __restrict__ at kernel level (as
// attn_append_body.h).  The includer defines
//   GQA_KERNEL  the extern "C" kernel name,
//   GQA_FP8     0: bf16 cache (GqaStripBf16);
//               1: FP8 KV cache (GqaStripFp8), and the kernel takes the
//                  exponent tensors Ke, Ve.
// No include guard: this file is meant to be included more than once.
#if GQA_FP8
#define GQA_ELEM unsigned char
#define GQA_STRIP GqaStripFp8
#define GQA_LOAD(st, base) \
  (st).load(Kb, Vb, Keb, Veb, rs, Hkv, base, r1, lane)
#else
#define GQA_ELEM unsigned short
#define GQA_STRIP GqaStripBf16
#define GQA_LOAD(st, base) (st).load(Kb, Vb, rs, base, r1, lane)
#endif
#define GQA_STEP(st, base) \
  gqa_step<GQA_FP8 != 0>(st, base, r1, q_b, qscale, m, l, o, vt, lane)
extern "C" __global__ __launch_bounds__(256, 2) void GQA_KERNEL(
    const unsigned short* __restrict__ qkv,  // [n, (Hq+2*Hkv)*128] raw
    GQA_ELEM* __restrict__ Kc,               // [slots, S_max, Hkv, 128]
    GQA_ELEM* __restrict__ Vc,
#if GQA_FP8
    unsigned char* __restrict__ Ke,          // [slots, S_max, Hkv]
    unsigned char* __restrict__ Ve,
#endif
    unsigned short* __restrict__ O,          // [n, Hq, 128]
    float* __restrict__ Ow,                  // [n, Hq, splits, 128]
    float* __restrict__ MLw,                 // [n, Hq, splits, 2]
    const float* __restrict__ cos_tab,       // [S, 64]
    const float* __restrict__ sin_tab,
    const int* __restrict__ positions,       // [n]
    const int* __restrict__ kv_lens,         // [n] == positions + 1
    const int* __restrict__ slot_ids,        // [n] -> cache slot
    int S_max, int Hq, int Hkv, int R, float qscale) {
  __shared__ __attribute__((aligned(16))) float lds[4][GQA_WAVE_FLOATS];
  __shared__ float red_m[4][16], red_l[4][16];

  const int sp = blockIdx.x;
  const int kvh = blockIdx.y;
  const int bq = blockIdx.z;
  const int splits = gridDim.x;
  const int group = Hq / Hkv;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int kb = lane >> 4;
  const int lr = lane & 15;

  // Per-sequence scalars (SGPRs).  Rows 0..p-1 come from the cache.
  const int slot = __builtin_amdgcn_readfirstlane(slot_ids[bq]);
  const int p = __builtin_amdgcn_readfirstlane(positions[bq]);
  const int nc = min(
      max(__builtin_amdgcn_readfirstlane(kv_lens[bq]) - 1, 0), S_max);
  const int r0 = sp * R;
  if (sp > 0 && r0 >= nc) return;  // empty split: writes nothing
  const int r1 = min(r0 + R, nc);

  const int heads = Hq + 2 * Hkv;
  const unsigned short* tok = qkv + (long long)bq * heads * GQA_D;

  // ---- Q^T as B fragments: lane holds q[head lr][d = 32ks + 8kb + j],
  // roped in fp32 (d and d + 64 are ks and ks + 2 of this lane), rounded
  // once to bf16.  Columns >= group are zero.
  s16x8 q_b[4];
  {
    float x[4][8];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) x[ks][j] = 0.f;
    if (lr < group) {
      const unsigned short* src =
          tok + (long long)(kvh * group + lr) * GQA_D + 8 * kb;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        bf8_to_f32(*(const s16x8*)(src + 32 * ks), x[ks]);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float cs[8], sn[8];
      const long long t = (long long)p * (GQA_D / 2) + 32 * h + 8 * kb;
      *(f32x4*)cs = *(const f32x4*)(cos_tab + t);
      *(f32x4*)(cs + 4) = *(const f32x4*)(cos_tab + t + 4);
      *(f32x4*)sn = *(const f32x4*)(sin_tab + t);
      *(f32x4*)(sn + 4) = *(const f32x4*)(sin_tab + t + 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        q_b[h][j] = (short)f2bf(x[h][j] * cs[j] - x[h + 2][j] * sn[j]);
        q_b[h + 2][j] = (short)f2bf(x[h + 2][j] * cs[j] + x[h][j] * sn[j]);
      }
    }
  }

  const long long slot_row0 = (long long)slot * S_max * Hkv + kvh;
  const long long rs = (long long)Hkv * GQA_D;  // elements per cache row
  GQA_ELEM* Kb = Kc + slot_row0 * GQA_D;
  GQA_ELEM* Vb = Vc + slot_row0 * GQA_D;
#if GQA_FP8
  unsigned char* Keb = Ke + slot_row0;
  unsigned char* Veb = Ve + slot_row0;
#endif

  // Softmax state of q head lr in log2 units; l is the lane's share of the
  // sum.  O^T: o[ct][r] = O[q = lr][d = 16ct + 4kb + r].
  float m = -INFINITY, l = 0.f;
  f32x4 o[8];
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) o[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  char* vt = (char*)lds[w];

  // ---- current token: split 0, wave 0.  The row layout of kv_fp8.h
  // (lane chunk c = lr, every lane group the same values) ropes k, writes
  // row p, and leaves the attended k and v as fp32 in the wave's LDS, from
  // where the lanes pick the elements of their fragments.
  if (sp == 0 && w == 0) {
    float cs[8], sn[8], kq[8], vq[8];
    {
      const long long t = (long long)p * (GQA_D / 2) + (lr & 7) * 8;
      *(f32x4*)cs = *(const f32x4*)(cos_tab + t);
      *(f32x4*)(cs + 4) = *(const f32x4*)(cos_tab + t + 4);
      *(f32x4*)sn = *(const f32x4*)(sin_tab + t);
      *(f32x4*)(sn + 4) = *(const f32x4*)(sin_tab + t + 4);
    }
    const unsigned short* kraw = tok + (long long)(Hq + kvh) * GQA_D;
    const unsigned short* vraw = tok + (long long)(Hq + Hkv + kvh) * GQA_D;
    gqa_rope8(kraw, lr, cs, sn, kq);
    const s16x8 vbits = *(const s16x8*)(vraw + lr * 8);
    bf8_to_f32(vbits, vq);
    const long long dst = (long long)p * Hkv;  // row p of (slot, kvh)
#if GQA_FP8
    float ak = 0.f, av = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ak = fmaxf(ak, fabsf(kq[j]));
      av = fmaxf(av, fabsf(vq[j]));
    }
    const int nk = kv8_exponent(row16_max(ak));
    const int nv = kv8_exponent(row16_max(av));
    const i32x2 kcode = kv8_quantize8(kq, nk);
    const i32x2 vcode = kv8_quantize8(vq, nv);
    kv8_decode8(kcode, kq);
    kv8_decode8(vcode, vq);
    const float sk = kv8_scale((unsigned)(nk + 127));
    const float sv = kv8_scale((unsigned)(nv + 127));
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // attended as code * 2^n
      kq[j] *= sk;
      vq[j] *= sv;
    }
    if (kb == 0) {
      *(i32x2*)(Kb + dst * GQA_D + lr * 8) = kcode;
      *(i32x2*)(Vb + dst * GQA_D + lr * 8) = vcode;
      if (lr == 0) {
        Keb[dst] = (unsigned char)(nk + 127);
        Veb[dst] = (unsigned char)(nv + 127);
      }
    }
#else
    if (kb == 0) {
      *(s16x8*)(Kb + dst * GQA_D + lr * 8) = f32_to_bf8(kq);
      *(s16x8*)(Vb + dst * GQA_D + lr * 8) = vbits;
    }
#endif
    float* cur = lds[0];  // k at [0, 128), v at [128, 256)
    if (kb == 0) {
      *(f32x4*)(cur + lr * 8) = f32x4{kq[0], kq[1], kq[2], kq[3]};
      *(f32x4*)(cur + lr * 8 + 4) = f32x4{kq[4], kq[5], kq[6], kq[7]};
      *(f32x4*)(cur + GQA_D + lr * 8) = f32x4{vq[0], vq[1], vq[2], vq[3]};
      *(f32x4*)(cur + GQA_D + lr * 8 + 4) =
          f32x4{vq[4], vq[5], vq[6], vq[7]};
    }
    float dot = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const f32x4 k0 = *(const f32x4*)(cur + 32 * ks + 8 * kb);
      const f32x4 k1 = *(const f32x4*)(cur + 32 * ks + 8 * kb + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dot += bf2f((unsigned short)q_b[ks][j]) * k0[j];
        dot += bf2f((unsigned short)q_b[ks][j + 4]) * k1[j];
      }
    }
    dot += __shfl_xor(dot, 16, 64);
    dot += __shfl_xor(dot, 32, 64);
    m = dot * qscale;
    l = (kb == 0) ? 1.f : 0.f;
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
      o[ct] = *(const f32x4*)(cur + GQA_D + 16 * ct + 4 * kb);
  }

  // ---- the row loop: strips w, w+4, ... of [r0, r1), loads one strip
  // ahead in the other register set.
  const int nstrips = (r1 - r0 + GQA_STRIP_ROWS - 1) / GQA_STRIP_ROWS;
  if (w < nstrips) {
    GQA_STRIP sa, sb;
    int s = w;
    GQA_LOAD(sa, r0 + GQA_STRIP_ROWS * s);
    for (;;) {
      bool last = s + 4 >= nstrips;
      GQA_LOAD(sb, r0 + GQA_STRIP_ROWS * (last ? s : s + 4));
      GQA_STEP(sa, r0 + GQA_STRIP_ROWS * s);
      if (last) break;
      s += 4;
      last = s + 4 >= nstrips;
      GQA_LOAD(sa, r0 + GQA_STRIP_ROWS * (last ? s : s + 4));
      GQA_STEP(sb, r0 + GQA_STRIP_ROWS * s);
      if (last) break;
      s += 4;
    }
  }

  // ---- the four waves meet in LDS: O^T partial as [q][d], m and l.
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  {
    float* ow = lds[w];
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
      *(f32x4*)(ow + lr * GQA_O_STRIDE + 16 * ct + 4 * kb) = o[ct];
    if (kb == 0) {
      red_m[w][lr] = m;
      red_l[w][lr] = l;
    }
  }
  __syncthreads();
  const int col = tid >> 4;  // q head of the group
  const int c = tid & 15;    // d = 8c .. 8c+7
  if (col >= group) return;
  float gm = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) gm = fmaxf(gm, red_m[i][col]);
  float gl = 0.f, a[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float mi = red_m[i][col];
    const float cc = (mi == -INFINITY) ? 0.f : gqa_exp2(mi - gm);
    gl += red_l[i][col] * cc;
    const float* src = lds[i] + col * GQA_O_STRIDE + 8 * c;
    const f32x4 x0 = *(const f32x4*)src;
    const f32x4 x1 = *(const f32x4*)(src + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] += x0[j] * cc;
      a[j + 4] += x1[j] * cc;
    }
  }
  const long long row = (long long)bq * Hq + kvh * group + col;
  if (splits == 1) {
    const float inv = (gl > 0.f) ? 1.f / gl : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] *= inv;
    *(s16x8*)(O + row * GQA_D + 8 * c) = f32_to_bf8(a);
    return;
  }
  float* dstp = Ow + (row * splits + sp) * GQA_D + 8 * c;
  *(f32x4*)dstp = f32x4{a[0], a[1], a[2], a[3]};
  *(f32x4*)(dstp + 4) = f32x4{a[4], a[5], a[6], a[7]};
  if (c == 0) {
    MLw[(row * splits + sp) * 2] = gm;
    MLw[(row * splits + sp) * 2 + 1] = gl;
  }
}
#undef GQA_ELEM
#undef GQA_STRIP
#undef GQA_LOAD
#undef GQA_STEP
