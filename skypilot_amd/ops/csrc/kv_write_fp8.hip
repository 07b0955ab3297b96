// Quantising KV-cache write for prefill and chunked prefill (FP8 KV cache,
// kv_fp8.h): rows i < lens[b] of k, v [n, S, Hkv, 128] bf16 go to
// [slot_ids[b], starts[b] + i] of the code and exponent tensors, the whole
// batch in one launch.
//
// Sixteen lanes per row: a 16-byte load, a 4-step DPP amax, four packed
// conversions, an 8-byte store; lane 0 of the row stores the exponent
// byte.  blockIdx.y picks K or V.  slot, start and length come from device
// tensors (no host sync).  The append kernel's rules decide what is
// skipped, and nothing else is written: rows at or past lens[b], rows that
// would land at or past S_max, and every row of a sequence whose slot is
// outside [0, slots) or whose start is negative.
#include "kv_fp8.h"

extern "C" __global__ __launch_bounds__(256) void kv_write_fp8_kernel(
    const unsigned short* __restrict__ k,   // [n, S, Hkv, 128]
    const unsigned short* __restrict__ v,
    unsigned char* __restrict__ Kc,         // [slots, S_max, Hkv, 128]
    unsigned char* __restrict__ Vc,
    unsigned char* __restrict__ Ke,         // [slots, S_max, Hkv]
    unsigned char* __restrict__ Ve,
    const int* __restrict__ slot_ids, const int* __restrict__ starts,
    const int* __restrict__ lens, long long rows, int S, int Hkv, int slots,
    int S_max) {
  const int c = threadIdx.x & 15;  // 8-element chunk of the row
  const long long row = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (row >= rows) return;  // whole 16-lane rows leave together
  const int h = (int)(row % Hkv);
  const long long tok = row / Hkv;
  const int i = (int)(tok % S);
  const int b = (int)(tok / S);
  const int slot = slot_ids[b];
  const int start = starts[b];
  const long long dst_row = (long long)start + i;
  if (i >= lens[b] || slot < 0 || slot >= slots || start < 0 ||
      dst_row >= S_max)
    return;

  const unsigned short* src = (blockIdx.y ? v : k) + row * KV8_D + c * 8;
  const s16x8 raw = *(const s16x8*)src;
  float x[8];
  bf8_to_f32(raw, x);
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(x[j]));
  amax = row16_max(amax);
  const int n = kv8_exponent(amax);
  const i32x2 codes = kv8_quantize8(x, n);

  const long long dst = ((long long)slot * S_max + dst_row) * Hkv + h;
  *(i32x2*)((blockIdx.y ? Vc : Kc) + dst * KV8_D + c * 8) = codes;
  if (c == 0) (blockIdx.y ? Ve : Ke)[dst] = (unsigned char)(n + 127);
}

extern "C" void kv_write_fp8_launch(const void* k, const void* v, void* Kc,
                                    void* Vc, void* Ke, void* Ve,
                                    const int* slot_ids, const int* starts,
                                    const int* lens, int n, int S, int Hkv,
                                    int slots, int S_max,
                                    hipStream_t stream) {
  const long long rows = (long long)n * S * Hkv;
  dim3 grid((unsigned)((rows + 15) / 16), 2);
  hipLaunchKernelGGL(kv_write_fp8_kernel, grid, dim3(256), 0, stream,
                     (const unsigned short*)k, (const unsigned short*)v,
                     (unsigned char*)Kc, (unsigned char*)Vc,
                     (unsigned char*)Ke, (unsigned char*)Ve, slot_ids, starts,
                     lens, rows, S, Hkv, slots, S_max);
}
