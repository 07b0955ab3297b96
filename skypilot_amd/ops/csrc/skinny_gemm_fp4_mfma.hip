// MXFP4-weight decode GEMM on the matrix cores, 1 <= n <= 64 tokens:
//   Y[t,o] = bf16( sum_k X[t,k] * e2m1(code[o,k]) * 2^(exps[o,k/32]-127) ),
// fp32 accumulate.  Weights are OCP MXFP4: two e2m1 codes per byte (element
// 2j in bits 0..3 of byte j, 2j+1 in bits 4..7) and one E8M0 exponent byte
// per block of 32 consecutive k of a row: 4.25 bits per weight.
//
// v_cvt_scalef32_pk_bf16_fp4 turns one byte (two codes) into two bf16 and
// multiplies them by a float scale in the same VALU op, so MX block
// dequantisation costs what the fp8 kernel's plain conversion costs per
// weight.  code * 2^n is exact in bf16: this is a bf16 MFMA GEMM over
// exactly dequantised weights.
//
// Operands are swapped as in skinny_gemm_fp8_mfma.hip (Y^T = W * X^T): 16 W
// rows are the A operand, 16 tokens the B columns, a lane's four C registers
// are four consecutive output features of one token (one 8-byte store; there
// is no row scale).
//
// Work split.  A 256-thread block owns TR tiles of 16 output rows; its four
// waves split K: wave w takes the 128-wide k chunks w, w+4, w+8, ...  Each
// wave keeps TR x NT accumulator tiles (NT = ceil(n/16)) and the partials
// meet in LDS in the fixed order ((w0+w1)+w2)+w3.  The k order depends on I
// alone: a token's output bits do not depend on n, NT, TR or its column.
//
// Data movement.  One 16-byte nontemporal load per lane is 32 codes = one MX
// block, so a wave load covers 16 rows x 128 k (a whole chunk, four MFMA
// k-steps) and the lane needs exactly one scale for it.  Lane (row r = l&15,
// group g = l>>4) holds codes k0 + 32g .. 32g+31 of row r; dword s of its 16
// bytes is its A fragment of k-step s (four cvts, byte selects 0..3).  So
// MFMA k index (g, j) of step s is memory k0 + 32g + 8s + j, and the B
// fragment of lane (token t = l&15, g) is the 16 bytes of X[t] at the same
// k: the four steps are 64 contiguous bytes of X[t].  The four exponent
// bytes of (row r, chunk) are one aligned dword (I % 128 == 0); every lane
// loads it with the W load it belongs to, picks byte g and forms the float
// as e << 23.  W and exps go straight to registers, never LDS.  Padding
// columns n..16*NT-1 are zero fragments; no address past row n-1 of X is
// formed.
//
// Pipeline.  vmcnt retires loads in issue order, so loads are issued in the
// order they are consumed: X steps 2,3 of this chunk, W and scales of the
// wave's next chunk (in flight under the MFMAs), X steps 0,1 of the next.
#include "common.h"

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// 8 e2m1 codes (one dword, memory order) times `scale` -> 8 bf16.
__device__ __forceinline__ bf16x8 fp4x8_to_bf16(unsigned d, float scale) {
  union {
    bf16x2 p[4];
    bf16x8 v;
  } u;
  u.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 0);
  u.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 1);
  u.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 2);
  u.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 3);
  return u.v;
}

// One chunk (128 k) of W for a lane: the lane's MX block and the dword of
// the chunk's four exponent bytes, per row tile.
template <int TR>
struct W4Chunk {
  i32x4 w[TR];
  unsigned e[TR];
};
// Half a chunk (64 k, two k-steps) of X for a lane: column tile nt, step s.
template <int NT>
struct X4Half {
  s16x8 x[NT][2];
};

template <int NT, int TR>
__global__ __launch_bounds__(256, 2) void skinny_gemm_fp4_mfma_kernel(
    const unsigned char* __restrict__ W4, const unsigned char* __restrict__ E,
    const unsigned short* __restrict__ X, unsigned short* __restrict__ Y,
    int n, int I, int O) {
  __shared__ f32x4 red[4][TR * NT][WAVE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int ntiles = O >> 4, nchunks = I >> 7;
  const int tile0 = blockIdx.x * TR;

  // Row tiles past the end (last block, TR > 1) stream the last tile again
  // and are never stored.
  const unsigned char* wp[TR];
  const unsigned char* ep[TR];
#pragma unroll
  for (int tr = 0; tr < TR; ++tr) {
    const int tile = tile0 + tr < ntiles ? tile0 + tr : ntiles - 1;
    const long long row = tile * 16 + r;
    wp[tr] = W4 + row * (I >> 1) + g * 16;
    ep[tr] = E + row * (I >> 5);
  }
  const unsigned short* xp[NT];
  bool live[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int t = nt * 16 + r;
    live[nt] = t < n;
    xp[nt] = X + (live[nt] ? (long long)t * I + g * 32 : 0);
  }

  // Chunk c of a row: code bytes 64c .. 64c+63, exponent bytes 4c .. 4c+3.
  auto load_w = [&](W4Chunk<TR>& d, int c) {
#pragma unroll
    for (int tr = 0; tr < TR; ++tr) {
      d.w[tr] = __builtin_nontemporal_load((const i32x4*)(wp[tr] + c * 64));
      d.e[tr] = __builtin_nontemporal_load((const unsigned*)(ep[tr] + c * 4));
    }
  };
  auto load_x = [&](X4Half<NT>& d, int c, int h) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const s16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
      d.x[nt][0] = d.x[nt][1] = zero;
      if (live[nt]) {
        const s16x8* p = (const s16x8*)(xp[nt] + c * 128 + h * 16);
        d.x[nt][0] = p[0];
        d.x[nt][1] = p[1];
      }
    }
  };

  f32x4 acc[TR][NT];
#pragma unroll
  for (int tr = 0; tr < TR; ++tr)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[tr][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // k-steps 2h and 2h+1 of a chunk.
  auto mma_half = [&](const W4Chunk<TR>& wc, int h, const X4Half<NT>& xh) {
#pragma unroll
    for (int tr = 0; tr < TR; ++tr) {
      const float sc = __uint_as_float(((wc.e[tr] >> (8 * g)) & 0xffu) << 23);
      bf16x8 a0 = fp4x8_to_bf16((unsigned)wc.w[tr][2 * h], sc);
      bf16x8 a1 = fp4x8_to_bf16((unsigned)wc.w[tr][2 * h + 1], sc);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        acc[tr][nt] = MFMA_BF16(a0, as_bf16x8(xh.x[nt][0]), acc[tr][nt]);
        acc[tr][nt] = MFMA_BF16(a1, as_bf16x8(xh.x[nt][1]), acc[tr][nt]);
      }
    }
  };

  W4Chunk<TR> wc, wn;
  X4Half<NT> xa, xb;
  int c = wave;
  if (c < nchunks) {
    load_w(wc, c);
    load_x(xa, c, 0);
  }
  for (; c < nchunks; c += 4) {
    const bool more = c + 4 < nchunks;
    load_x(xb, c, 1);
    if (more) load_w(wn, c + 4);
    mma_half(wc, 0, xa);
    if (more) load_x(xa, c + 4, 0);
    mma_half(wc, 1, xb);
    if (more) wc = wn;
  }

  // Fixed-order split-K reduction; wave w finishes tiles w, w+4, ...
#pragma unroll
  for (int tr = 0; tr < TR; ++tr)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) red[wave][tr * NT + nt][lane] = acc[tr][nt];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < (TR * NT + 3) / 4; ++i) {
    const int ti = wave + 4 * i;
    if (ti >= TR * NT) break;
    const int tile = tile0 + ti / NT, t = (ti % NT) * 16 + r;
    f32x4 s = ((red[0][ti][lane] + red[1][ti][lane]) + red[2][ti][lane]) +
              red[3][ti][lane];
    if (tile < ntiles && t < n) {
      const int o = tile * 16 + g * 4;
      i32x2 out;
      out[0] = (int)((unsigned)f2bf(s[0]) | ((unsigned)f2bf(s[1]) << 16));
      out[1] = (int)((unsigned)f2bf(s[2]) | ((unsigned)f2bf(s[3]) << 16));
      *(i32x2*)(Y + (long long)t * O + o) = out;
    }
  }
}

// Row tiles per wave (TR = 1, 2 or 4; the output bits do not depend on it).
// Every block reads all of X from L2, n*I*2 bytes against 8*TR*I bytes of W
// (twice the fp8 kernel's ratio), so more column tiles want more row tiles
// per block; fewer blocks in turn leave fewer loads in flight.  row_tiles = 0
// picks the measured best (bench_gemm_fp4_mfma.py, docs/BENCHMARKS.md).
extern "C" void skinny_gemm_fp4_mfma_launch(const void* W4, const void* E,
                                            const void* X, void* Y, int n,
                                            int I, int O, int row_tiles,
                                            hipStream_t stream) {
  const int ntiles = O / 16, nt = (n + 15) / 16;
  int tr = row_tiles;
  // Measured: 4 wins or ties at every n on O = 28672 and 128256, 2 at every
  // n on O = 6144, 1 on O = 4096 (256 tiles, one per CU) at either I.
  if (tr == 0) tr = O >= 16384 ? 4 : O >= 6144 ? 2 : 1;
  dim3 grid((ntiles + tr - 1) / tr), block(256);
#define MFMA_CASE(NT, TR)                                                  \
  hipLaunchKernelGGL((skinny_gemm_fp4_mfma_kernel<NT, TR>), grid, block, 0, \
                     stream, (const unsigned char*)W4,                     \
                     (const unsigned char*)E, (const unsigned short*)X,    \
                     (unsigned short*)Y, n, I, O)
#define MFMA_NT(NT)          \
  case NT:                   \
    if (tr == 4)             \
      MFMA_CASE(NT, 4);      \
    else if (tr == 2)        \
      MFMA_CASE(NT, 2);      \
    else                     \
      MFMA_CASE(NT, 1);      \
    break;
  switch (nt) {
    MFMA_NT(1) MFMA_NT(2) MFMA_NT(3) MFMA_NT(4)
    default:
      break;  // the binding guarantees 1 <= n <= 64
  }
#undef MFMA_NT
#undef MFMA_CASE
}
