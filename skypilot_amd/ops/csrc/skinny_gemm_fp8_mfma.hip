// FP8-weight decode GEMM on the matrix cores, 1 <= n <= 64 tokens:
//   Y[t,o] = bf16( scale[o] * sum_k X[t,k] * e4m3(W8[o,k]) ),  fp32 accumulate.
//
// The fp8 GEMV (skinny_gemm.hip) loses from n = 3 up because its unpack
// and dot work is VALU work that grows with n.  Here the only per-weight
// VALU work is the fp8 -> bf16 conversion (v_cvt_scalef32_pk_bf16_fp8, two
// elements per instruction; e4m3 is exact in bf16), and it is shared by
// every token: the multiply-adds are 16x16x32 bf16 MFMAs.
//
// Operands are swapped (Y^T = W * X^T): 16 W rows are the A operand, 16
// tokens the B columns, so a lane's four C registers are four consecutive
// output features of one token (one 8-byte store, row scale applied there).
//
// Work split.  A 256-thread block owns TR tiles of 16 output rows; its four
// waves split K: wave w takes the 128-wide k chunks w, w+4, w+8, ...  Each
// wave keeps TR x NT accumulator tiles (NT = ceil(n/16) column tiles) and
// the four partial sums meet in LDS in the fixed order ((w0+w1)+w2)+w3.
// The order in which k is accumulated therefore depends on I alone: a
// token's output bits do not depend on n, NT, TR or its column.
//
// Data movement.  W is read once from HBM: one 16-byte nontemporal load per
// lane covers 16 rows x 64 codes, straight into registers, never LDS.  Lane
// (row r = l&15, group g = l>>4) holds codes k0 + 16g .. 16g+15 of row r;
// codes 8s..8s+7 are its A fragment for k-step s = 0, 1.  So MFMA k index
// (g, j) of step s is memory k0 + 16g + 8s + j, and the B fragment of lane
// (token t = l&15, g) is the 16 bytes of X at the same k: both fragments of
// one 64-k unit are 32 contiguous bytes of X[t].  Every converted A
// fragment feeds all NT column tiles, and every B fragment all TR row
// tiles.  X (L2-resident) is read once per block, not once per wave.
// Padding columns n..16*NT-1 are zero fragments; no address past row n-1
// of X is formed.
//
// Pipeline.  vmcnt retires loads in issue order, so loads are issued in
// the order they are consumed: X unit 1 of this chunk, W of the wave's
// next chunk (2*TR loads in flight under the MFMAs), X unit 0 of the next.
#include "common.h"

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// 8 e4m3 codes (two dwords, memory order) -> 8 bf16.
__device__ __forceinline__ bf16x8 fp8x8_to_bf16(unsigned lo, unsigned hi) {
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

// One chunk (128 k) of W for a lane: unit u, row tile tr.
template <int TR>
struct WChunk {
  i32x4 w[2][TR];
};
// One unit (64 k) of X for a lane: column tile nt, k-step s.
template <int NT>
struct XUnit {
  s16x8 x[NT][2];
};

template <int NT, int TR>
__global__ __launch_bounds__(256, 2) void skinny_gemm_fp8_mfma_kernel(
    const unsigned char* __restrict__ W8, const float* __restrict__ scale,
    const unsigned short* __restrict__ X, unsigned short* __restrict__ Y,
    int n, int I, int O) {
  __shared__ f32x4 red[4][TR * NT][WAVE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int ntiles = O >> 4, nchunks = I >> 7;
  const int tile0 = blockIdx.x * TR;

  // Row tiles past the end (last block, TR = 2) stream the last tile
  // again and are never stored.
  const unsigned char* wp[TR];
#pragma unroll
  for (int tr = 0; tr < TR; ++tr) {
    int tile = tile0 + tr < ntiles ? tile0 + tr : ntiles - 1;
    wp[tr] = W8 + (long long)(tile * 16 + r) * I + g * 16;
  }
  const unsigned short* xp[NT];
  bool live[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    int t = nt * 16 + r;
    live[nt] = t < n;
    xp[nt] = X + (live[nt] ? (long long)t * I + g * 16 : 0);
  }

  auto load_w = [&](WChunk<TR>& d, int c) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int tr = 0; tr < TR; ++tr)
        d.w[u][tr] = __builtin_nontemporal_load(
            (const i32x4*)(wp[tr] + c * 128 + u * 64));
  };
  auto load_x = [&](XUnit<NT>& d, int c, int u) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const s16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
      d.x[nt][0] = d.x[nt][1] = zero;
      if (live[nt]) {
        const s16x8* p = (const s16x8*)(xp[nt] + c * 128 + u * 64);
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

  auto mma_unit = [&](const i32x4* w, const XUnit<NT>& xu) {
#pragma unroll
    for (int tr = 0; tr < TR; ++tr) {
      bf16x8 a0 = fp8x8_to_bf16((unsigned)w[tr][0], (unsigned)w[tr][1]);
      bf16x8 a1 = fp8x8_to_bf16((unsigned)w[tr][2], (unsigned)w[tr][3]);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        acc[tr][nt] = MFMA_BF16(a0, as_bf16x8(xu.x[nt][0]), acc[tr][nt]);
        acc[tr][nt] = MFMA_BF16(a1, as_bf16x8(xu.x[nt][1]), acc[tr][nt]);
      }
    }
  };

  WChunk<TR> wc, wn;
  XUnit<NT> xa, xb;
  int c = wave;
  if (c < nchunks) {
    load_w(wc, c);
    load_x(xa, c, 0);
  }
  for (; c < nchunks; c += 4) {
    const bool more = c + 4 < nchunks;
    load_x(xb, c, 1);
    if (more) load_w(wn, c + 4);
    mma_unit(wc.w[0], xa);
    if (more) load_x(xa, c + 4, 0);
    mma_unit(wc.w[1], xb);
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
      const f32x4 sc = *(const f32x4*)(scale + o);
      i32x2 out;
      out[0] = (int)((unsigned)f2bf(s[0] * sc[0]) |
                     ((unsigned)f2bf(s[1] * sc[1]) << 16));
      out[1] = (int)((unsigned)f2bf(s[2] * sc[2]) |
                     ((unsigned)f2bf(s[3] * sc[3]) << 16));
      *(i32x2*)(Y + (long long)t * O + o) = out;
    }
  }
}

// Row tiles per wave (TR = 1, 2 or 4; the output bits do not depend on it).
// Every block reads all of X from L2, n*I*2 bytes against 16*TR*I bytes of
// W, so more column tiles want more row tiles per block; fewer blocks in
// turn leave fewer loads in flight.  row_tiles = 0 picks the measured best
// (bench_gemm_fp8_mfma.py, docs/BENCHMARKS.md).
extern "C" void skinny_gemm_fp8_mfma_launch(const void* W8, const float* scale,
                                            const void* X, void* Y, int n,
                                            int I, int O, int row_tiles,
                                            hipStream_t stream) {
  const int ntiles = O / 16, nt = (n + 15) / 16;
  int tr = row_tiles;
  // Measured: 4 wins at every n on O = 28672 and 128256; on O = 6144 2 wins
  // from n = 32 up and ties 1 at 16; O = 4096 (256 tiles, one per CU) wants 1.
  if (tr == 0) tr = O >= 16384 ? 4 : (O >= 6144 && nt >= 2) ? 2 : 1;
  dim3 grid((ntiles + tr - 1) / tr), block(256);
#define MFMA_CASE(NT, TR)                                                  \
  hipLaunchKernelGGL((skinny_gemm_fp8_mfma_kernel<NT, TR>), grid, block, 0, \
                     stream, (const unsigned char*)W8, scale,              \
                     (const unsigned short*)X, (unsigned short*)Y, n, I, O)
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
