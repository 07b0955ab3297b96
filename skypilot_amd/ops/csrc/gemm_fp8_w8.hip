// FP8-weight GEMM for any token count (prefill, prompt chunks, verify steps
// and decode batches above 64):
//   Y[t,o] = bf16( scale[o] * sum_k X[t,k] * e4m3(W8[o,k]) ),  fp32 accumulate,
// n >= 1, I % 128 == 0, O % 64 == 0.  The product is skinny_gemm_fp8_mfma's:
// bf16 X, e4m3 codes converted exactly to bf16 (v_cvt_scalef32_pk_bf16_fp8,
// scale 1.0), 16x16x32 bf16 MFMAs, row scale and one bf16 rounding at the
// store.  That kernel stops at 64 tokens because every wave reads its X
// fragments from L2 itself; here the X tile is staged once per block in LDS
// and shared by the four waves.
//
// Operands are swapped (Y^T = W X^T): 16 W rows are A, 16 tokens the B
// columns, so a lane's four C registers are four consecutive output features
// of one token: the row scales are one 16-byte load, the result one 8-byte
// store.
//
// Work split.  A 256-thread block owns 64*TR features x 128 tokens, grid
// (ceil(O / (64*TR)), ceil(n / 128)).  Wave w owns the TR 16-row tiles
// 4*TR*bx + TR*w + tr and all 8 token tiles: TR x 8 accumulator tiles.  No
// split K: one accumulator chain per element, k ascending, so a token's
// output bits depend on I alone, not on n, its neighbours, TR or the grid.
//
// W path.  Global -> registers, nontemporal, never LDS, read once per token
// tile.  Lane (row r = l&15, group g = l>>4) holds, per 64-k unit u, the 16
// codes k0 + 64u + 16g .. +15 of row r; codes 8s..8s+7 are its A fragment
// for k-step s.  MFMA k index (g, j) of (u, s) is memory k0 + 64u + 16g + 8s
// + j, and the B fragment of lane (token r, g) is the 16 bytes of X[t] at the
// same k.  The loads of chunk c+1 are issued at the top of chunk c, right
// behind the barrier, and stay in flight under its MFMAs.
//
// X path.  Per 128-k chunk the X tile is 128 tokens x 256 B = 32 KB,
// double-buffered in LDS (64 KB) by 16-byte global_load_lds DMAs: linear
// destination, swizzled source.  A row holds 16 pieces of 16 B; piece
// q = 8u + 2g + s of token row R lives in LDS column q ^ (R & 15).  A fragment
// read is one ds_read_b128 whose 16 rows (R & 15 = r) are what varies in the
// instruction, so 16 lanes of a group hit 16 different 16-byte columns of a
// 256-byte span and any aligned 8 of them 8 different columns.  DMA ii of
// wave w fills LDS bytes (4*ii + w)*1024 + 16*lane: token row 16*ii + 4*w + g,
// column r, so the source piece is r ^ (4*w + g) whatever ii.
//
// Synchronisation: one vm_drain + barrier per chunk.  After it chunk c has
// landed (every wave drains its own DMAs) and every wave is done reading the
// other buffer.  The compiler orders an LDS read behind every LDS DMA in
// flight, so the chunk's fragment reads are issued before the next chunk's
// DMAs: the reads are software-pipelined one k-step ahead of the MFMAs and the
// DMAs follow the last read, in flight under the second half of the chunk's
// MFMAs.  Staging is unconditional: the last iteration restages its own chunk
// into the buffer nobody reads.
//
// Edges.  Token rows >= n are never addressed: the staged row is clamped to
// n - 1 (its columns are computed and not stored).  Row tiles past O / 16
// (TR = 2, O % 128 == 64) stream the last tile again and are not stored.
#include "common.h"

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

#define W8_TOK 128   // tokens per block and k per chunk

__device__ __forceinline__ void w8_gload_lds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)g,
      (__attribute__((address_space(3))) unsigned int*)l, 16, 0, 0);
}
// LDS-DMA completion is tracked by vmcnt; the barrier's own wait is not.
__device__ __forceinline__ void w8_vm_drain() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// 8 e4m3 codes (two dwords, memory order) -> 8 bf16.
__device__ __forceinline__ bf16x8 w8_fp8x8_to_bf16(unsigned lo, unsigned hi) {
  union {
    bf16x2 p[4];
    bf16x8 v;
  } u;
  u.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
  u.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
  u.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
  u.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
  return u.v;
}

template <int TR>
__global__ __launch_bounds__(256, 2) void gemm_fp8_w8_kernel(
    const unsigned char* __restrict__ W8, const float* __restrict__ scale,
    const unsigned short* __restrict__ X, unsigned short* __restrict__ Y,
    int n, int I, int O) {
  __shared__ __attribute__((aligned(1024))) unsigned char x_lds[2][W8_TOK * 256];

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int ntiles = O >> 4, nchunks = I >> 7;
  const int tile0 = ((int)blockIdx.x * 4 + wave) * TR;
  const long long t0 = (long long)blockIdx.y * W8_TOK;

  const unsigned char* wp[TR];
#pragma unroll
  for (int tr = 0; tr < TR; ++tr) {
    const int tile = tile0 + tr < ntiles ? tile0 + tr : ntiles - 1;
    wp[tr] = W8 + (long long)(tile * 16 + r) * I + g * 16;
  }
  // Staging plan: DMA ii of this wave moves piece r ^ srow of token row
  // 16*ii + srow (clamped to n - 1) to LDS column r of that row.
  const int srow = 4 * wave + g;
  const unsigned char* xsrc[8];
#pragma unroll
  for (int ii = 0; ii < 8; ++ii) {
    long long row = t0 + 16 * ii + srow;
    if (row > n - 1) row = n - 1;
    xsrc[ii] = (const unsigned char*)X + row * I * 2 + ((r ^ srow) << 4);
  }
  auto stage = [&](int buf, int c) {
#pragma unroll
    for (int ii = 0; ii < 8; ++ii)
      w8_gload_lds16(xsrc[ii] + (long long)c * 256,
                     x_lds[buf] + (4 * ii + wave) * 1024);
  };

  struct WChunk {
    i32x4 w[2][TR];   // [unit u][row tile]
  };
  auto load_w = [&](WChunk& d, int c) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int tr = 0; tr < TR; ++tr)
        d.w[u][tr] = __builtin_nontemporal_load(
            (const i32x4*)(wp[tr] + (long long)c * 128 + u * 64));
  };

  // Fragment read of k-step q = 2u + s, token tile nt: row 16*nt + r, piece
  // 8u + 2g + s = (2g) | (8u + s), column piece ^ r.
  const int b_row = r * 256, b_col = (2 * g) ^ r;
  auto read_x = [&](s16x8* x, int buf, int q) {
    const int off = b_row + ((b_col ^ ((q >> 1) * 8 + (q & 1))) << 4);
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
      x[nt] = *(const s16x8*)(x_lds[buf] + nt * 4096 + off);
  };

  f32x4 acc[TR][8];
#pragma unroll
  for (int tr = 0; tr < TR; ++tr)
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) acc[tr][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto mma = [&](const WChunk& wc, int q, const s16x8* x) {
#pragma unroll
    for (int tr = 0; tr < TR; ++tr) {
      const i32x4 w = wc.w[q >> 1][tr];
      const bf16x8 a = w8_fp8x8_to_bf16((unsigned)w[2 * (q & 1)],
                                        (unsigned)w[2 * (q & 1) + 1]);
#pragma unroll
      for (int nt = 0; nt < 8; ++nt)
        acc[tr][nt] = MFMA_BF16(a, as_bf16x8(x[nt]), acc[tr][nt]);
    }
  };

  WChunk wc, wn;
  load_w(wn, 0);
  stage(0, 0);
  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    const int cn = c + 1 < nchunks ? c + 1 : c;
    w8_vm_drain();
    __syncthreads();
    // The drain has landed this chunk's W too.  It is taken over here, not at
    // the end of the last iteration, where the copy would wait for the loads
    // and the DMAs in the middle of the MFMAs.
    wc = wn;
    load_w(wn, cn);
    __builtin_amdgcn_sched_barrier(0);
    s16x8 xa[8], xb[8];
    read_x(xa, buf, 0);
    read_x(xb, buf, 1);
    mma(wc, 0, xa);
    read_x(xa, buf, 2);
    mma(wc, 1, xb);
    read_x(xb, buf, 3);
    // The scheduling fences keep the DMAs behind the last fragment read and
    // in front of the second half of the MFMAs.
    __builtin_amdgcn_sched_barrier(0);
    stage(buf ^ 1, cn);
    __builtin_amdgcn_sched_barrier(0);
    mma(wc, 2, xa);
    mma(wc, 3, xb);
  }
  w8_vm_drain();  // the restaged tile must land before the LDS is released

#pragma unroll
  for (int tr = 0; tr < TR; ++tr) {
    if (tile0 + tr >= ntiles) continue;
    const int o = (tile0 + tr) * 16 + g * 4;
    const f32x4 sc = *(const f32x4*)(scale + o);
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
      const long long t = t0 + nt * 16 + r;
      if (t >= n) continue;
      const f32x4 s = acc[tr][nt];
      i32x2 out;
      out[0] = (int)((unsigned)f2bf(s[0] * sc[0]) |
                     ((unsigned)f2bf(s[1] * sc[1]) << 16));
      out[1] = (int)((unsigned)f2bf(s[2] * sc[2]) |
                     ((unsigned)f2bf(s[3] * sc[3]) << 16));
      *(i32x2*)(Y + t * O + o) = out;
    }
  }
}

// row_tiles: 16-row tiles per wave, 1 or 2 (the output bits do not depend on
// it); 0 picks by shape.  TR = 2 halves the X bytes a block stages per W byte
// but a block then takes 1.35x as long, so it is taken only where TR = 1 would
// need more blocks than the 512 the machine holds at once (256 CUs x 2).
// Measured: TR = 1 wins wherever its grid fits (0.73x-0.95x the time of
// TR = 2), TR = 2 wherever it does not (0.80x-0.95x); bench_gemm_fp8_prefill.py,
// docs/BENCHMARKS.md.
extern "C" void gemm_fp8_w8_launch(const void* W8, const float* scale,
                                   const void* X, void* Y, int n, int I, int O,
                                   int row_tiles, hipStream_t stream) {
  const int ntok = (n + W8_TOK - 1) / W8_TOK;
  int tr = row_tiles;
  if (tr == 0) tr = (long long)(O / 64) * ntok > 512 ? 2 : 1;
  const int rows = 64 * tr;
  dim3 grid((O + rows - 1) / rows, ntok), block(256);
  if (tr == 2)
    hipLaunchKernelGGL((gemm_fp8_w8_kernel<2>), grid, block, 0, stream,
                       (const unsigned char*)W8, scale,
                       (const unsigned short*)X, (unsigned short*)Y, n, I, O);
  else
    hipLaunchKernelGGL((gemm_fp8_w8_kernel<1>), grid, block, 0, stream,
                       (const unsigned char*)W8, scale,
                       (const unsigned short*)X, (unsigned short*)Y, n, I, O);
}
