// Fused rope + cache write + decode attention over the FP8 KV cache
// (kv_fp8.h): the fp8 twin of attn_decode_qkv_kernel (attention_decode.hip),
// same call contract, one 256-thread block per (sequence, q head).
//
// Semantics: attention sees the dequantised rows, the current token
// included.  The current k is roped in fp32 and quantised in registers,
// the current v is quantised from the raw bf16; both are attended as
// code * 2^n, and one designated block per kv head (qh % group == 0)
// stores the codes and the two exponent bytes at (slot, p).  So the output
// equals "write row p, then attend rows 0..p" and no block reads row p.
//
// Row loop.  A 128-byte row is 16 lanes x 8 bytes, so one wave load covers
// four rows (lane group g = lane >> 4 takes row base + 4u + g, chunk
// c = lane & 15) and the dot product is reduced with four DPP steps inside
// the 16-lane row instead of six wave shuffles.  Each lane group is its
// own online-softmax chain (four per wave, sixteen per block, merged at the
// end), and a chain advances four rows per step with ONE rescale: scores
// d_0..d_3 first, then m' = max(m, d_u), o = o * e^(m - m') + sum_u
// e^(d_u - m') 2^nv_u code_u.  The K scale multiplies the reduced partial
// sum and the V scale multiplies the weight; both are powers of two, so
// this is exact.  The exponent bytes are one byte load per row group.
// Every loop is bounded by kv_len - 1; the tail clamps the row index to the
// last valid cache row and masks the score, so no row at or past kv_len - 1
// is read (those rows may hold NaN codes and exponent 0xFF).
#include "kv_fp8.h"

// Rope of the 8 elements [8c, 8c+8) of a head: own chunk and the chunk 64
// elements away (c ^ 8); cs/sn are table entries 8 * (c & 7) + j.
__device__ __forceinline__ void rope8(const unsigned short* head, int c,
                                      const float* cs, const float* sn,
                                      float* out) {
  float own[8], par[8];
  bf8_to_f32(*(const s16x8*)(head + c * 8), own);
  bf8_to_f32(*(const s16x8*)(head + (c ^ 8) * 8), par);
  const float sgn = (c < 8) ? -1.f : 1.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = own[j] * cs[j] + sgn * par[j] * sn[j];
}

extern "C" __global__ __launch_bounds__(256) void attn_decode_qkv_fp8_kernel(
    const unsigned short* __restrict__ qkv,  // [B, (Hq+2*Hkv)*128] raw
    unsigned char* __restrict__ Kc,          // [slots, S_max, Hkv, 128]
    unsigned char* __restrict__ Vc,
    unsigned char* __restrict__ Ke,          // [slots, S_max, Hkv]
    unsigned char* __restrict__ Ve,
    unsigned short* __restrict__ O,          // [B, Hq, 128]
    const float* __restrict__ cos_tab,       // [S, 64]
    const float* __restrict__ sin_tab,
    const int* __restrict__ positions,       // [B]
    const int* __restrict__ kv_lens,         // [B] == positions + 1
    const int* __restrict__ slot_ids,        // [B] -> cache slot
    int B, int S_max, int Hq, int Hkv, float scale) {
  const int bq = blockIdx.x / Hq;
  const int b = slot_ids ? slot_ids[bq] : bq;
  const int qh = blockIdx.x % Hq;
  const int group = Hq / Hkv;
  const int kvh = qh / group;
  const int kv_len = kv_lens[bq];
  const int p = positions[bq];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int g = lane >> 4;  // row of the wave load, and softmax chain
  const int c = lane & 15;  // 8-element chunk of the row

  float cs[8], sn[8];
  {
    const long long t = (long long)p * (KV8_D / 2) + (c & 7) * 8;
    *(f32x4*)cs = *(const f32x4*)(cos_tab + t);
    *(f32x4*)(cs + 4) = *(const f32x4*)(cos_tab + t + 4);
    *(f32x4*)sn = *(const f32x4*)(sin_tab + t);
    *(f32x4*)(sn + 4) = *(const f32x4*)(sin_tab + t + 4);
  }
  const int heads = Hq + 2 * Hkv;
  const unsigned short* qraw = qkv + ((long long)bq * heads + qh) * KV8_D;
  const unsigned short* kraw =
      qkv + ((long long)bq * heads + Hq + kvh) * KV8_D;
  const unsigned short* vraw =
      qkv + ((long long)bq * heads + Hq + Hkv + kvh) * KV8_D;

  // roped q (pre-scaled); current k and v quantised, then dequantised.
  float q[8], kq[8], vq[8];
  rope8(qraw, c, cs, sn, q);
#pragma unroll
  for (int j = 0; j < 8; ++j) q[j] *= scale;
  rope8(kraw, c, cs, sn, kq);
  bf8_to_f32(*(const s16x8*)(vraw + c * 8), vq);
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
  const float sk_cur = kv8_scale((unsigned)(nk + 127));
  const float sv_cur = kv8_scale((unsigned)(nv + 127));

  const long long slot_row0 = (long long)b * S_max * Hkv + kvh;
  // cache write for future steps: one block per kv head, 16 lanes.
  if (qh % group == 0 && w == 0 && g == 0) {
    const long long dst = slot_row0 + (long long)p * Hkv;
    *(i32x2*)(Kc + dst * KV8_D + c * 8) = kcode;
    *(i32x2*)(Vc + dst * KV8_D + c * 8) = vcode;
    if (c == 0) {
      Ke[dst] = (unsigned char)(nk + 127);
      Ve[dst] = (unsigned char)(nv + 127);
    }
  }

  float m = -INFINITY, l = 0.f, o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = 0.f;
  {
    // wave 0, chain 0: seed with the current token.
    float dc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) dc += q[j] * kq[j];
    dc = row16_sum(dc) * sk_cur;
    if (w == 0 && g == 0) {
      m = dc;
      l = 1.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = vq[j] * sv_cur;
    }
  }

  const int n_cache = kv_len - 1;  // rows 0..p-1 come from the cache
  const long long rs = (long long)Hkv * KV8_D;
  const unsigned char* Kb = Kc + slot_row0 * KV8_D + c * 8;
  const unsigned char* Vb = Vc + slot_row0 * KV8_D + c * 8;
  const unsigned char* Keb = Ke + slot_row0;
  const unsigned char* Veb = Ve + slot_row0;
  for (int base = w * 16; base < n_cache; base += 64) {
    const bool full = base + 16 <= n_cache;  // wave-uniform
    i32x2 kw[4], vw[4];
    unsigned ke[4], ve[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = base + 4 * u + g;
      ok[u] = full || row < n_cache;
      const long long rc = full ? row : min(row, n_cache - 1);
      kw[u] = *(const i32x2*)(Kb + rc * rs);
      ke[u] = Keb[rc * Hkv];
      vw[u] = *(const i32x2*)(Vb + rc * rs);
      ve[u] = Veb[rc * Hkv];
    }
    float d[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float f[8];
      kv8_decode8(kw[u], f);
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += q[j] * f[j];
      d[u] = acc;
    }
    // four interleaved 16-lane reductions
#pragma unroll
    for (int u = 0; u < 4; ++u) d[u] += kv8_dpp<0xB1>(d[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) d[u] += kv8_dpp<0x4E>(d[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) d[u] += kv8_dpp<0x141>(d[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) d[u] += kv8_dpp<0x140>(d[u]);
    float mn = m;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      d[u] = ok[u] ? d[u] * kv8_scale(ke[u]) : -INFINITY;
      mn = fmaxf(mn, d[u]);
    }
    const float cr = (m == -INFINITY) ? 0.f : __expf(m - mn);
    l *= cr;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] *= cr;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float e = ok[u] ? __expf(d[u] - mn) : 0.f;
      const float ev = ok[u] ? e * kv8_scale(ve[u]) : 0.f;
      float f[8];
      kv8_decode8(vw[u], f);
      l += e;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] += ev * f[j];
    }
    m = mn;
  }

  // merge the wave's four chains (lane groups) ...
  float gm = fmaxf(m, __shfl_xor(m, 16, 64));
  gm = fmaxf(gm, __shfl_xor(gm, 32, 64));
  {
    const float cc = (m == -INFINITY) ? 0.f : __expf(m - gm);
    l *= cc;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] *= cc;
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    o[j] += __shfl_xor(o[j], 16, 64);
    o[j] += __shfl_xor(o[j], 32, 64);
  }
  // ... and the four waves through LDS.
  __shared__ float red_m[4], red_l[4];
  __shared__ __attribute__((aligned(16))) float red_o[4][KV8_D];
  if (lane == 0) {
    red_m[w] = gm;
    red_l[w] = l;
  }
  if (g == 0) {
    *(f32x4*)&red_o[w][c * 8] = f32x4{o[0], o[1], o[2], o[3]};
    *(f32x4*)&red_o[w][c * 8 + 4] = f32x4{o[4], o[5], o[6], o[7]};
  }
  __syncthreads();
  if (tid < 16) {
    float bm = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) bm = fmaxf(bm, red_m[i]);
    float gl = 0.f, a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float cc = (red_m[i] == -INFINITY) ? 0.f : __expf(red_m[i] - bm);
      gl += red_l[i] * cc;
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += red_o[i][c * 8 + j] * cc;
    }
    const float inv = (gl > 0.f) ? 1.f / gl : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] *= inv;
    *(s16x8*)(O + ((long long)bq * Hq + qh) * KV8_D + c * 8) = f32_to_bf8(a);
  }
}

extern "C" void attn_decode_qkv_fp8_launch(
    const void* qkv, void* Kc, void* Vc, void* Ke, void* Ve, void* O,
    const void* cos_tab, const void* sin_tab, const int* positions,
    const int* kv_lens, const int* slot_ids, int B, int S_max, int Hq,
    int Hkv, float scale, hipStream_t stream) {
  hipLaunchKernelGGL(attn_decode_qkv_fp8_kernel, dim3(B * Hq), dim3(256), 0,
                     stream, (const unsigned short*)qkv, (unsigned char*)Kc,
                     (unsigned char*)Vc, (unsigned char*)Ke,
                     (unsigned char*)Ve, (unsigned short*)O,
                     (const float*)cos_tab, (const float*)sin_tab, positions,
                     kv_lens, slot_ids, B, S_max, Hq, Hkv, scale);
}
