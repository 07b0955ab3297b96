// MXFP4-weight x MXFP8-activation prefill GEMM on the block-scaled MFMA:
//   Y[t,o] = bf16( sum_k e4m3(xq[t,k]) * 2^(xe[t,k/32]-127)
//                      * e2m1(code[o,k]) * 2^(exps[o,k/32]-127) ),
// fp32 accumulate, any n >= 1, I % 128 == 0, O % 128 == 0.  Two kernels:
// quantize_mxfp8_rows_kernel turns bf16 X into MXFP8 (ops.quantize_mxfp8 is
// the definition, reproduced bit for bit), gemm_mxfp4_a8_kernel contracts it
// with the MXFP4 weights of ops.quantize_mxfp4 through
// v_mfma_scale_f32_16x16x128_f8f6f4.  Every product is exact in fp32; the
// only roundings are the accumulation and the final bf16.
//
// Operands are swapped as in the decode siblings (Y^T = W X^T): 16 W rows
// are A (fp4, cbsz = 4: 4 VGPRs), 16 tokens the B columns (e4m3, blgp = 0:
// 8 VGPRs).  Measured layout of the 16x16x128 form, lane (row l&15, group
// g = l>>4): the fp4 operand holds k 32g..32g+31 (one MX block, the 16-byte
// load skinny_gemm_fp4_mfma makes); the fp8 operand holds k 16g..16g+15 in
// registers 0..3 and k 64+16g..64+16g+15 in registers 4..7 (two 16-byte
// pieces 64 k apart, from two different MX blocks); the scale of (row, block
// b) comes from lane group b for both, whichever lanes hold the block's
// data.  test_one_hot_rows_return_the_weights pins all of it.  A lane's four
// C registers are four consecutive output features of one token: one 8-byte
// store.
//
// Work split.  A 256-thread block owns 128 features x 128 tokens, waves
// 2 x 2, 64 x 64 per wave = 16 accumulator tiles.  One k chunk of 128 is
// 16 MFMAs per wave from 4 A and 4 B fragments.  No split K: one
// accumulator chain per element, k order a function of I alone, so a
// token's output bits do not depend on n, its neighbours or the grid.
//
// Data movement.  Per chunk the W tile is 128 rows x 64 B, the X tile 128
// rows x 128 B, double-buffered in LDS (48 KB) by 16-byte global_load_lds
// DMAs: linear destination, swizzled source.  Fragment reads are
// ds_read_b128 from rows 64 B (W) or 128 B (X) apart, where the 16 rows of a
// fragment are what varies within the instruction, so the XOR keys on row
// bits 0..3.  Slot = chunk ^ f(row) with
//   W (4 slots of 16 B a row):  f = ((row >> 2) ^ (row & 2)) & 3
//   X (8 slots of 16 B a row):  f = ((row >> 1) & 7) ^ ((row & 1) << 2)
// Both send 16 consecutive rows at a fixed chunk to 16 different 16-byte
// columns of a 256-byte span and any aligned 8 of them to 8 different
// columns of a 128-byte span: conflict-free whether the hardware serves a
// b128 read 8 or 16 lanes at a time.  The four exponent bytes of (row,
// chunk) are one aligned dword, loaded straight to registers one chunk
// ahead; the lane picks byte g and packs its four fragments' bytes into one
// VGPR, the MFMA's opsel picks the fragment.  The quantiser pads X to whole
// token tiles (zero codes, exponent 127), so no load is clamped or masked;
// stores are masked by t < n.
#include "common.h"

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

#define A8_TILE 128   // features and tokens per block, k per chunk

__device__ __forceinline__ void a8_gload_lds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)g,
      (__attribute__((address_space(3))) unsigned int*)l, 16, 0, 0);
}
// LDS-DMA completion is tracked by vmcnt; the barrier's own wait is not.
__device__ __forceinline__ void a8_vm_drain() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ int a8_swz_w(int row) {
  return ((row >> 2) ^ (row & 2)) & 3;
}
__device__ __forceinline__ int a8_swz_x(int row) {
  return ((row >> 1) & 7) ^ ((row & 1) << 2);
}

// ---------------------------------------------------------------------------
// Quantiser: one lane owns one block of 32 values (four 16-byte loads, two
// 16-byte stores, amax lane-local).  n comes from the bf16 bits of amax: with
// a = max |x| as bf16 bits, n = (a >> 7) - 135 + (mantissa > 0x60), clamped
// to [-100, 100], 0 for a == 0.  v_cvt_scalef32_pk_fp8_bf16 with scale 2^n
// gives e4m3fn(x / 2^n), round to nearest even, subnormals and ties as
// torch's conversion has them (measured: bit-equal to ops.quantize_mxfp8 on
// its edge blocks and on random data; the scale operand divides).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void quantize_mxfp8_rows_kernel(
    const unsigned short* __restrict__ X, unsigned char* __restrict__ Q,
    unsigned char* __restrict__ E, int n, int n_pad, int I) {
  const int bpr = I >> 5;
  const long long nblk = (long long)n_pad * bpr;
  for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < nblk;
       b += (long long)gridDim.x * 256) {
    const long long row = b / bpr;
    i32x4 out[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    unsigned char eb = 127;
    if (row < n) {
      const s16x8* p = (const s16x8*)(X + b * 32);
      s16x8 v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = p[i];
      unsigned a = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          a = max(a, (unsigned)(unsigned short)v[i][j] & 0x7fffu);
      int e = (int)(a >> 7) - 135 + ((a & 0x7fu) > 0x60u ? 1 : 0);
      e = min(max(e, -100), 100);
      if (a == 0) e = 0;
      eb = (unsigned char)(e + 127);
      const float sc = __uint_as_float((unsigned)(e + 127) << 23);   // 2^n
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          typedef __attribute__((ext_vector_type(2))) short v2s;
          union { unsigned u; bf16x2 b; } lo, hi;
          union { v2s s; unsigned u; } w;
          lo.u = (unsigned short)v[i][4 * d] |
                 ((unsigned)(unsigned short)v[i][4 * d + 1] << 16);
          hi.u = (unsigned short)v[i][4 * d + 2] |
                 ((unsigned)(unsigned short)v[i][4 * d + 3] << 16);
          w.u = 0;
          w.s = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(w.s, lo.b, sc, false);
          w.s = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(w.s, hi.b, sc, true);
          out[i >> 1][(i & 1) * 2 + d] = (int)w.u;
        }
    }
    i32x4* q = (i32x4*)(Q + b * 32);
    q[0] = out[0];
    q[1] = out[1];
    E[b] = eb;
  }
}

// ---------------------------------------------------------------------------
// GEMM.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void gemm_mxfp4_a8_kernel(
    const unsigned char* __restrict__ W4, const unsigned char* __restrict__ WE,
    const unsigned char* __restrict__ XQ, const unsigned char* __restrict__ XE,
    unsigned short* __restrict__ Y, int n, int I, int O) {
  __shared__ __attribute__((aligned(1024))) unsigned char w_lds[2][128 * 64];
  __shared__ __attribute__((aligned(1024))) unsigned char x_lds[2][128 * 128];

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const long long o0 = (long long)blockIdx.x * A8_TILE;
  const long long t0 = (long long)blockIdx.y * A8_TILE;
  const int nchunks = I >> 7, epr = I >> 5;

  // Staging plan: DMA ii of wave w fills LDS slots (4*ii + w)*64 + lane.
  const unsigned char* wbase = W4 + o0 * (I >> 1);
  const unsigned char* xbase = XQ + t0 * I;
  unsigned wsrc[2], xsrc[4];
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) {
    const int s = (4 * ii + wave) * 64 + lane, row = s >> 2;
    wsrc[ii] = (unsigned)row * (unsigned)(I >> 1) +
               (((s & 3) ^ a8_swz_w(row)) << 4);
  }
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int s = (4 * ii + wave) * 64 + lane, row = s >> 3;
    xsrc[ii] = (unsigned)row * (unsigned)I + (((s & 7) ^ a8_swz_x(row)) << 4);
  }
  auto stage = [&](int buf, int c) {
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
      a8_gload_lds16(wbase + c * 64 + wsrc[ii],
                     w_lds[buf] + (4 * ii + wave) * 1024);
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
      a8_gload_lds16(xbase + c * 128 + xsrc[ii],
                     x_lds[buf] + (4 * ii + wave) * 1024);
  };

  // Exponent dwords of the wave's 4 + 4 fragment rows, chunk c.
  const unsigned char* wep = WE + (o0 + wm * 64 + r) * epr;
  const unsigned char* xep = XE + (t0 + wn * 64 + r) * epr;
  struct Scales {
    unsigned a[4], b[4];
  };
  auto load_scales = [&](Scales& s, int c) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s.a[i] = *(const unsigned*)(wep + (long long)i * 16 * epr + c * 4);
      s.b[i] = *(const unsigned*)(xep + (long long)i * 16 * epr + c * 4);
    }
  };

  // Fragment read offsets: the swizzle keys on row bits 0..3 = r only.
  const int a_off = (wm * 64 + r) * 64 + ((g ^ a8_swz_w(r)) << 4);
  const int b_off = (wn * 64 + r) * 128 + ((g ^ a8_swz_x(r)) << 4);

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  Scales nxt;
  stage(0, 0);
  load_scales(nxt, 0);
  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    // Chunk c has landed in buf (every wave drains its own DMAs), and every
    // wave is done reading buf ^ 1.
    a8_vm_drain();
    __syncthreads();
    const Scales cur = nxt;
    unsigned sa = 0, sb = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sa |= ((cur.a[i] >> (8 * g)) & 0xffu) << (8 * i);
      sb |= ((cur.b[i] >> (8 * g)) & 0xffu) << (8 * i);
    }
    // Fragment reads come before the next chunk's DMAs are issued: the
    // compiler orders an LDS read after every LDS DMA in flight (vmcnt(0)),
    // so reads issued behind the staging would wait for it.
    i32x8 a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const i32x4 lo = *(const i32x4*)(w_lds[buf] + a_off + i * 1024);
      a[i] = i32x8{lo[0], lo[1], lo[2], lo[3], 0, 0, 0, 0};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const i32x4 lo = *(const i32x4*)(x_lds[buf] + b_off + j * 2048);
      const i32x4 hi = *(const i32x4*)(x_lds[buf] + (b_off ^ 64) + j * 2048);
      b[j] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
    // Unconditional: the last iteration restages its own chunk into the
    // buffer nobody reads.  The scheduling fences keep the DMAs and the
    // scale loads in front of the MFMAs, a whole chunk ahead of their use.
    const int cn = c + 1 < nchunks ? c + 1 : c;
    __builtin_amdgcn_sched_barrier(0);
    stage(buf ^ 1, cn);
    load_scales(nxt, cn);
    __builtin_amdgcn_sched_barrier(0);
#define A8_MFMA(i, j)                                                  \
  acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(        \
      a[i], b[j], acc[i][j], 4, 0, i, (int)sa, j, (int)sb)
#define A8_ROW(i) A8_MFMA(i, 0); A8_MFMA(i, 1); A8_MFMA(i, 2); A8_MFMA(i, 3)
    A8_ROW(0); A8_ROW(1); A8_ROW(2); A8_ROW(3);
#undef A8_ROW
#undef A8_MFMA
  }
  a8_vm_drain();  // the restaged tile must land before the LDS is released

#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long t = t0 + wn * 64 + j * 16 + r;
    if (t >= n) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long o = o0 + wm * 64 + i * 16 + g * 4;
      const f32x4 s = acc[i][j];
      i32x2 out;
      out[0] = (int)((unsigned)f2bf(s[0]) | ((unsigned)f2bf(s[1]) << 16));
      out[1] = (int)((unsigned)f2bf(s[2]) | ((unsigned)f2bf(s[3]) << 16));
      *(i32x2*)(Y + t * O + o) = out;
    }
  }
}

// X [n, I] bf16 -> Q [n_pad, I] e4m3fn, E [n_pad, I/32]; n_pad = n rounded up
// to A8_TILE.
extern "C" void quantize_mxfp8_rows_launch(const void* X, void* Q, void* E,
                                           int n, int n_pad, int I,
                                           hipStream_t stream) {
  const long long nblk = (long long)n_pad * (I / 32);
  dim3 grid(membound_grid(nblk, 256)), block(256);
  hipLaunchKernelGGL(quantize_mxfp8_rows_kernel, grid, block, 0, stream,
                     (const unsigned short*)X, (unsigned char*)Q,
                     (unsigned char*)E, n, n_pad, I);
}

extern "C" void gemm_mxfp4_a8_launch(const void* W4, const void* WE,
                                     const void* XQ, const void* XE, void* Y,
                                     int n, int n_pad, int I, int O,
                                     hipStream_t stream) {
  dim3 grid(O / A8_TILE, n_pad / A8_TILE), block(256);
  hipLaunchKernelGGL(gemm_mxfp4_a8_kernel, grid, block, 0, stream,
                     (const unsigned char*)W4, (const unsigned char*)WE,
                     (const unsigned char*)XQ, (const unsigned char*)XE,
                     (unsigned short*)Y, n, I, O);
}
