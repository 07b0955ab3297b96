// FP8 KV-cache row format, shared by kv_write_fp8.hip,
// attention_decode_fp8.hip and attention_append.hip (docs/KERNELS.md,
// "FP8 KV cache").
//
// A row is the 128 values of one (token, kv head), K or V.  It is stored
// as 128 OCP e4m3fn codes and one E8M0 exponent byte e, scale 2^(e-127).
// With amax = max |x_i| in fp32, n is the smallest integer with
// amax <= 448 * 2^n, clamped to [-126, 127] (0 for amax == 0), e = n + 127
// and code_i = e4m3fn(x_i * 2^-n), round to nearest even.  Both scalings
// are by a power of two, hence exact: codes and exponent are a pure
// function of the inputs, and code * 2^n is exactly representable in bf16.
//
// Sixteen lanes hold one row, eight consecutive elements each; the row
// reductions below are DPP steps inside that 16-lane row (no LDS).
#pragma once

#include "common.h"

#define KV8_D 128

// x from another lane of the same 16-lane row.  quad_perm [1,0,3,2],
// quad_perm [2,3,0,1], row_half_mirror, row_mirror: applied in this order
// with a commutative op they leave the full 16-lane result in every lane,
// bit-identical across the lanes.
template <int CTRL>
__device__ __forceinline__ float kv8_dpp(float x) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL,
                                         0xf, 0xf, true));
}

__device__ __forceinline__ float row16_sum(float x) {
  x += kv8_dpp<0xB1>(x);
  x += kv8_dpp<0x4E>(x);
  x += kv8_dpp<0x141>(x);
  x += kv8_dpp<0x140>(x);
  return x;
}

__device__ __forceinline__ float row16_max(float x) {
  x = fmaxf(x, kv8_dpp<0xB1>(x));
  x = fmaxf(x, kv8_dpp<0x4E>(x));
  x = fmaxf(x, kv8_dpp<0x141>(x));
  x = fmaxf(x, kv8_dpp<0x140>(x));
  return x;
}

// n from the fp32 bits of amax >= 0: 448 = 1.75 * 2^8 and 0x600000 is the
// mantissa of 1.75.  No division, no log.  NaN/Inf give n <= 127, so the
// exponent byte never reaches 255.
__device__ __forceinline__ int kv8_exponent(float amax) {
  const unsigned u = __builtin_bit_cast(unsigned, amax) & 0x7fffffffu;
  int n = (int)(u >> 23) - 135 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
  n = min(max(n, -126), 127);
  return u == 0u ? 0 : n;
}

// 2^(e-127) for an exponent byte of a stored row (1 <= e <= 254).
__device__ __forceinline__ float kv8_scale(unsigned e) {
  return __builtin_bit_cast(float, e << 23);
}

// Eight fp32 values of a row with exponent n -> eight e4m3fn codes.
__device__ __forceinline__ i32x2 kv8_quantize8(const float* x, int n) {
  float y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) y[j] = __builtin_ldexpf(x[j], -n);  // exact
  i32x2 w;
  int a = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
  w[0] = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], a, true);
  int b = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false);
  w[1] = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], b, true);
  return w;
}

// Eight codes -> their fp32 values (unscaled).
__device__ __forceinline__ void kv8_decode8(i32x2 w, float* out) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[h], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[h], true);
    out[4 * h + 0] = lo[0];
    out[4 * h + 1] = lo[1];
    out[4 * h + 2] = hi[0];
    out[4 * h + 3] = hi[1];
  }
}

// Eight codes times the row scale -> eight bf16.  code * 2^n has at most
// four significant bits, so dropping the low fp32 half is exact.
__device__ __forceinline__ s16x8 kv8_dequant_bf16(i32x2 w, float scale) {
  float f[8];
  kv8_decode8(w, f);
  s16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (short)f2bf_trunc(f[j] * scale);
  return r;
}

#include "kv_fp8_launch.h"
