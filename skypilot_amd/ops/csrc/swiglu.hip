// Fused SwiGLU forward/backward for CDNA4 (gfx950).
//
// Input is the fused gate|up GEMM output gu [rows, 2M] (gate = first M
// columns): y = silu(g) * u.  Backward writes dgu [rows, 2M] in one
// pass, eliminating the eager silu/mul kernels and the backward
// torch.cat observed in the r01 profile.  Memory-bound; s16x8 loads.
#include "common.h"

__device__ __forceinline__ float sigmoidf_(float x) {
  return 1.f / (1.f + __expf(-x));
}

extern "C" __global__ void swiglu_fwd_kernel(
    const unsigned short* __restrict__ gu, unsigned short* __restrict__ y,
    long long rows, int M) {
  const int nvec = M / 8;
  const long long total = rows * nvec;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = i0; i < total; i += stride) {
    long long row = i / nvec;
    int v = (int)(i % nvec);
    const s16x8 gv = *(const s16x8*)(gu + row * 2 * M + v * 8);
    const s16x8 uv = *(const s16x8*)(gu + row * 2 * M + M + v * 8);
    float out[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float g = bf2f((unsigned short)gv[j]);
      float u = bf2f((unsigned short)uv[j]);
      out[j] = g * sigmoidf_(g) * u;
    }
    *(s16x8*)(y + row * M + v * 8) = f32_to_bf8(out);
  }
}

// dg, du for eight elements: the one definition both backward kernels use.
__device__ __forceinline__ void swiglu_bwd_vec(const s16x8 gv, const s16x8 uv,
                                               const s16x8 dyv, float* dg,
                                               float* du) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float g = bf2f((unsigned short)gv[j]);
    float u = bf2f((unsigned short)uv[j]);
    float d = bf2f((unsigned short)dyv[j]);
    float sg = sigmoidf_(g);
    float silu = g * sg;
    dg[j] = d * u * (sg + silu * (1.f - sg));
    du[j] = d * silu;
  }
}

extern "C" __global__ void swiglu_bwd_kernel(
    const unsigned short* __restrict__ gu,
    const unsigned short* __restrict__ dy,
    unsigned short* __restrict__ dgu, long long rows, int M) {
  const int nvec = M / 8;
  const long long total = rows * nvec;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = i0; i < total; i += stride) {
    long long row = i / nvec;
    int v = (int)(i % nvec);
    const s16x8 gv = *(const s16x8*)(gu + row * 2 * M + v * 8);
    const s16x8 uv = *(const s16x8*)(gu + row * 2 * M + M + v * 8);
    const s16x8 dyv = *(const s16x8*)(dy + row * M + v * 8);
    float dg[8], du[8];
    swiglu_bwd_vec(gv, uv, dyv, dg, du);
    *(s16x8*)(dgu + row * 2 * M + v * 8) = f32_to_bf8(dg);
    *(s16x8*)(dgu + row * 2 * M + M + v * 8) = f32_to_bf8(du);
  }
}

// ---------------------------------------------------------------------------
// swiglu_bwd that also writes dguT [2M, rows] = dgu^T, the operand layout of
// weight-gradient routes 1 and 2 (bindings.cpp linear_wgrad), from the
// registers that hold dgu: the separate transpose_bf16 pass over dgu (one
// more read and the same write) goes away.  One wave per 64x64 tile of the
// gate half and the matching tile of the up half.  Lane (g, s) = (lane >> 3,
// lane & 7) owns rows 8g.., columns 8s.. of both tiles, so the eight lanes of
// one g read and write whole 128-byte lines; the values are
// swiglu_bwd_kernel's (swiglu_bwd_vec).  Each half then goes through
// transpose_bf16_kernel's recipe (wgrad_gemm.hip): v_perm_b32 transposes the
// lane's 8x8 block, the block lands in a [out row][64] LDS image with the
// 16-byte chunk index XORed with (out row >> 3), and comes back with g and s
// swapped so that a store again covers whole lines of dguT.  8 KB of LDS,
// used for the gate tile and then for the up tile.
// ---------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// out[c][r] = v's 64x64 tile transposed; out points at dguT[c0][r0], R is
// dguT's row length.
__device__ __forceinline__ void store_tile_transposed(
    const u32x4 (&v)[8], u32x4* t, unsigned short* out, long long R, int g,
    int s) {
  __syncthreads();  // the previous image's LDS reads are done
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    // out row 8s + i holds v's rows 8g .. 8g+7 at column 8s + i: chunk g
    const unsigned sel = (i & 1) ? 0x07060302u : 0x05040100u;
    u32x4 o;
#pragma unroll
    for (int m = 0; m < 4; ++m)
      o[m] = __builtin_amdgcn_perm(v[2 * m + 1][i >> 1], v[2 * m][i >> 1],
                                   sel);
    t[(8 * s + i) * 8 + (g ^ s)] = o;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = g + 8 * i;  // out row of the tile; c >> 3 == i
    *(u32x4*)(out + c * R + 8 * s) = t[c * 8 + (s ^ i)];
  }
}

extern "C" __global__ __launch_bounds__(64) void swiglu_bwd_t_kernel(
    const unsigned short* __restrict__ gu,
    const unsigned short* __restrict__ dy, unsigned short* __restrict__ dgu,
    unsigned short* __restrict__ dguT, int rows, int M) {
  __shared__ u32x4 t[64 * 8];  // [out row][chunk ^ (out row >> 3)]
  const int tiles_r = rows >> 6;
  const int tiles_c = M >> 6;
  const int g = threadIdx.x >> 3;
  const int s = threadIdx.x & 7;
  const long long R = rows;
  for (long long tile = blockIdx.x; tile < (long long)tiles_r * tiles_c;
       tile += gridDim.x) {
    const long long r0 = (tile / tiles_c) << 6;
    const long long c0 = (tile % tiles_c) << 6;
    u32x4 dgv[8], duv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long row = r0 + 8 * g + j;
      const long long col = c0 + 8 * s;
      const s16x8 gv = *(const s16x8*)(gu + row * 2 * M + col);
      const s16x8 uv = *(const s16x8*)(gu + row * 2 * M + M + col);
      const s16x8 dyv = *(const s16x8*)(dy + row * M + col);
      float dg[8], du[8];
      swiglu_bwd_vec(gv, uv, dyv, dg, du);
      const s16x8 dgb = f32_to_bf8(dg);
      const s16x8 dub = f32_to_bf8(du);
      *(s16x8*)(dgu + row * 2 * M + col) = dgb;
      *(s16x8*)(dgu + row * 2 * M + M + col) = dub;
      dgv[j] = __builtin_bit_cast(u32x4, dgb);
      duv[j] = __builtin_bit_cast(u32x4, dub);
    }
    store_tile_transposed(dgv, t, dguT + c0 * R + r0, R, g, s);
    store_tile_transposed(duv, t, dguT + (M + c0) * R + r0, R, g, s);
  }
}

extern "C" void swiglu_fwd_launch(const void* gu, void* y, long long rows,
                                  int M, hipStream_t stream) {
  int grid = membound_grid(rows * (M / 8), 256);
  hipLaunchKernelGGL(swiglu_fwd_kernel, dim3(grid), dim3(256), 0, stream,
                     (const unsigned short*)gu, (unsigned short*)y, rows, M);
}

extern "C" void swiglu_bwd_launch(const void* gu, const void* dy, void* dgu,
                                  long long rows, int M,
                                  hipStream_t stream) {
  int grid = membound_grid(rows * (M / 8), 256);
  hipLaunchKernelGGL(swiglu_bwd_kernel, dim3(grid), dim3(256), 0, stream,
                     (const unsigned short*)gu, (const unsigned short*)dy,
                     (unsigned short*)dgu, rows, M);
}

// rows and M are positive multiples of 64 and every pointer is 16-byte
// aligned (checked by the binding).
extern "C" void swiglu_bwd_t_launch(const void* gu, const void* dy, void* dgu,
                                    void* dguT, int rows, int M,
                                    hipStream_t stream) {
  long long tiles = ((long long)rows >> 6) * (M >> 6);
  // one wave per block; at 164 VGPRs three waves fit a SIMD, so 3072 blocks
  // are all resident on the 256 CUs
  int grid = tiles > 3072 ? 3072 : (int)tiles;
  hipLaunchKernelGGL(swiglu_bwd_t_kernel, dim3(grid), dim3(64), 0, stream,
                     (const unsigned short*)gu, (const unsigned short*)dy,
                     (unsigned short*)dgu, (unsigned short*)dguT, rows, M);
}
