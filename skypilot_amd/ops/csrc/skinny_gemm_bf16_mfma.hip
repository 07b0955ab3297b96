// bf16-weight decode GEMM on the matrix cores, 1 <= n <= 64 tokens:
//   Y[t,o] = bf16( sum_k X[t,k] * W[o,k] ),  fp32 accumulate,
// W the model's own [O, I] bf16 weight: no copy, no registration.
//
// Operands are swapped as in skinny_gemm_fp8_mfma.hip (Y^T = W * X^T): 16 W
// rows are the A operand of mfma_f32_16x16x32_bf16, 16 tokens the B columns,
// NT = ceil(n/16) column tiles, every A fragment feeds all of them.
//
// Work split.  Unlike the fp8 kernel the four waves of a block split the
// output rows, not K: wave w owns TR tiles of 16 rows over the block's whole
// k range, a block 64*TR rows, and nothing is reduced across waves.  K is
// split across blocks instead: grid (ceil(O / (64*TR)), KS), block (bx, ks)
// takes a contiguous range of 128-k chunks.  KS == 1 stores bf16 Y; KS > 1
// stores fp32 partials [KS, n, O] that skinny_gemm_bf16_combine_kernel sums
// in the order ks = 0, 1, ... (no atomics).  TR and KS are picked from (O, I)
// alone, so the k order behind an output element depends on the weight's
// shape only: a token's bits do not depend on n, NT or its neighbours.
//
// W path.  Global memory straight into A fragments: one nontemporal 16-byte
// load per lane is a fragment, lane (row r = l&15, group g = l>>4) holds
// k0 + 8g .. +7 of row r, a wave load covers 16 rows x 32 k.  Each wave keeps
// a ring of 8 k-steps x TR fragments: the loads of the next two 128-k chunks
// are in flight under the MFMAs of the current one, and a slot is reloaded,
// two chunks ahead, right after its MFMAs.  vmcnt retires in order, so loads
// are issued in the order they are consumed.  TR = 4, which only row_tiles=4
// reaches, keeps 4 x 4 fragments, one chunk ahead: two chunks deep it spills
// at NT = 4 (197 VGPRs, 344 B of scratch per lane by hipcc's resource
// remarks; 256 VGPRs at NT = 3).  Its speed at that depth was not measured.
//
// X path.  X crosses L2 once per block.  For each chunk, wave w loads the B
// fragments of k-step w (lane (token l&15, g) the 16 bytes at k0 + 32w + 8g;
// zeros for tokens >= n) into registers and writes them to LDS at
// [nt*4 + w][lane]: B-fragment order, so both the ds_write_b128 and every
// wave's ds_read_b128 touch 64 consecutive 16-byte slots and are free of
// bank conflicts.  Two LDS buffers, one barrier per chunk.  The registers
// are loaded as far ahead as the W ring (chunk c+2 before the W loads of
// chunk c+2) and written at the end of chunk c+1, so the wait before the
// write leaves two chunks of W in flight.  Staging goes through registers,
// so the barrier needs no vmcnt drain.
#include "skinny_gemm_bf16_mfma.h"

#include "common.h"

union w_frag {
  i32x4 i;
  bf16x8 b;
};

template <int NT, int TR>
__global__ __launch_bounds__(256, 2) void skinny_gemm_bf16_mfma_kernel(
    const unsigned short* __restrict__ W, const unsigned short* __restrict__ X,
    unsigned short* __restrict__ Y, float* __restrict__ P, int n, int I,
    int O) {
  __shared__ s16x8 xs[2][NT * 4][WAVE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int ntiles = O >> 4, nchunks = I >> 7;
  // Chunks [c0, c0 + nc) of this k split; nc may be 0 (KS > nchunks).  An
  // empty split takes c0 = 0, so that the pointers below stay inside W and
  // X although nothing is loaded through them.
  const int KS = gridDim.y, ks = blockIdx.y;
  const int base = nchunks / KS, rem = nchunks % KS;
  const int nc = base + (ks < rem ? 1 : 0);
  const int c0 = nc > 0 ? ks * base + (ks < rem ? ks : rem) : 0;
  const int tile0 = (blockIdx.x * 4 + wave) * TR;

  // Row tiles past the end (last block) stream the last tile again and are
  // never stored.
  const unsigned short* wp[TR];
#pragma unroll
  for (int tr = 0; tr < TR; ++tr) {
    const int tile = tile0 + tr < ntiles ? tile0 + tr : ntiles - 1;
    wp[tr] = W + (long long)(tile * 16 + r) * I + c0 * 128 + g * 8;
  }
  // Lanes of tokens >= n load row n - 1 again (a line their neighbours
  // fetch anyway) and stage zeros: no branch in the loop, and no address
  // past row n - 1 is formed.
  const unsigned short* xp[NT];
  bool live[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int t = nt * 16 + r;
    live[nt] = t < n;
    xp[nt] = X + (long long)(live[nt] ? t : n - 1) * I + c0 * 128 +
             wave * 32 + g * 8;
  }

  // D chunks of W (4*D k-steps x TR fragments) are in flight per wave; a
  // lane's X share is loaded D chunks ahead too, so that the wait for it
  // before the LDS write leaves the younger W loads in flight.  TR = 4
  // with D = 2 spills (see the top of the file).
  constexpr int D = TR == 4 ? 1 : 2;
  w_frag ring[D][4][TR];   // [chunk % D][k-step][row tile]
  s16x8 xr[D][NT];         // [chunk % D]: this wave's share of an X chunk
  f32x4 acc[TR][NT];
#pragma unroll
  for (int tr = 0; tr < TR; ++tr)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[tr][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // c: chunk relative to c0.  q (a slot of ring / xr) and b (an LDS buffer)
  // are constants at every call, so everything stays in registers.
  auto load_x = [&](int c, int q) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      xr[q][nt] = *(const s16x8*)(xp[nt] + c * 128);
  };
  auto store_x = [&](int q, int b) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      xs[b][nt * 4 + wave][lane] =
          live[nt] ? xr[q][nt] : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
  };
  auto load_w = [&](int c, int q, int s) {
#pragma unroll
    for (int tr = 0; tr < TR; ++tr)
      ring[q][s][tr].i = __builtin_nontemporal_load(
          (const i32x4*)(wp[tr] + c * 128 + s * 32));
  };
  auto read_b = [&](bf16x8* f, int b, int s) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) f[nt] = as_bf16x8(xs[b][nt * 4 + s][lane]);
  };
  // Chunk c of parity par.  next: chunk c + 1 exists, ahead: chunk c + D
  // exists.  The B fragments of k-step s + 1 are read under the MFMAs of
  // step s; each ring slot is reloaded, D chunks ahead, right after its
  // MFMAs.  The scheduling barriers keep the loads in the order written,
  // which is the order they are consumed in.
  auto chunk = [&](int c, int par, bool next, bool ahead) {
    const int q = par & (D - 1);
    if (ahead) load_x(c + D, q);
    bf16x8 f[2][NT];
    read_b(f[0], par, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s < 3) read_b(f[(s + 1) & 1], par, s + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int tr = 0; tr < TR; ++tr)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[tr][nt] = MFMA_BF16(ring[q][s][tr].b, f[s & 1][nt], acc[tr][nt]);
      if (ahead) load_w(c + D, q, s);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (next) {
      store_x((par + 1) & (D - 1), par ^ 1);
      __syncthreads();
    }
  };
  // X and W of the first D chunks, in consumption order.
  auto prologue = [&](bool full) {
    load_x(0, 0);
#pragma unroll
    for (int s = 0; s < 4; ++s) load_w(0, 0, s);
    if (D == 2 && full) {
      load_x(1, 1);
#pragma unroll
      for (int s = 0; s < 4; ++s) load_w(1, 1, s);
    }
    __builtin_amdgcn_sched_barrier(0);
    store_x(0, 0);
    __syncthreads();
  };

  // The steady loop is free of branches, so that the state of the vmcnt
  // queue at its head is the same from the prologue and from the back edge
  // and hipcc's waits are exact.  The last chunks, and ranges shorter than
  // four chunks, take the tail.
  int c = 0;
  if (nc >= 4) {
    prologue(true);
    for (; c + 1 + D < nc; c += 2) {
      chunk(c, 0, true, true);
      chunk(c + 1, 1, true, true);
    }
  } else if (nc > 0) {
    prologue(nc > 1);
  }
  if (c < nc) chunk(c, 0, c + 1 < nc, c + D < nc);
  if (c + 1 < nc) chunk(c + 1, 1, c + 2 < nc, c + 1 + D < nc);
  if (c + 2 < nc) chunk(c + 2, 0, false, false);

  // Lane l's four C registers are features 4g .. 4g+3 of token l&15.
#pragma unroll
  for (int tr = 0; tr < TR; ++tr)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int tile = tile0 + tr, t = nt * 16 + r;
      if (tile < ntiles && t < n) {
        const int o = tile * 16 + g * 4;
        const f32x4 s = acc[tr][nt];
        if (KS == 1) {
          i32x2 out;
          out[0] = (int)((unsigned)f2bf(s[0]) | ((unsigned)f2bf(s[1]) << 16));
          out[1] = (int)((unsigned)f2bf(s[2]) | ((unsigned)f2bf(s[3]) << 16));
          *(i32x2*)(Y + (long long)t * O + o) = out;
        } else {
          *(f32x4*)(P + ((long long)ks * n + t) * O + o) = s;
        }
      }
    }
}

// Y = bf16(((P[0] + P[1]) + P[2]) + ...), four features per thread.
__global__ __launch_bounds__(256) void skinny_gemm_bf16_combine_kernel(
    const f32x4* __restrict__ P, unsigned short* __restrict__ Y, int quads,
    int KS) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= quads) return;
  f32x4 s = P[q];
  for (int ks = 1; ks < KS; ++ks) s += P[(long long)ks * quads + q];
  i32x2 out;
  out[0] = (int)((unsigned)f2bf(s[0]) | ((unsigned)f2bf(s[1]) << 16));
  out[1] = (int)((unsigned)f2bf(s[2]) | ((unsigned)f2bf(s[3]) << 16));
  *(i32x2*)(Y + 4 * (long long)q) = out;
}

// Row tiles per wave and k splits from the weight's shape alone (never from
// n: see above).  Measured on the five Llama-3-8B shapes
// (bench_gemm_bf16_mfma.py, docs/BENCHMARKS.md): the kernel is fastest at
// about one block per CU, 192 to 256 blocks where the shape allows; two row
// tiles won at O = 6144 and 28672, one at 4096 and, by 2.5 %, at 128256.
extern "C" void skinny_gemm_bf16_mfma_plan(int I, int O, int* row_tiles,
                                           int* k_splits) {
  (void)I;
  if (*row_tiles == 0) *row_tiles = O >= 6144 && O < 65536 ? 2 : 1;
  if (*k_splits == 0) {
    const int blocks = (O + 64 * *row_tiles - 1) / (64 * *row_tiles);
    int ks = 1;
    while (ks < 8 && blocks * ks < 192) ks *= 2;
    *k_splits = ks;
  }
}

extern "C" void skinny_gemm_bf16_mfma_launch(const void* W, const void* X,
                                             void* Y, float* partials, int n,
                                             int I, int O, int row_tiles,
                                             int k_splits,
                                             hipStream_t stream) {
  const int nt = (n + 15) / 16, tr = row_tiles, rows = 64 * tr;
  dim3 grid((O + rows - 1) / rows, k_splits), block(256);
#define MFMA_CASE(NT, TR)                                                    \
  hipLaunchKernelGGL((skinny_gemm_bf16_mfma_kernel<NT, TR>), grid, block, 0, \
                     stream, (const unsigned short*)W,                       \
                     (const unsigned short*)X, (unsigned short*)Y, partials, \
                     n, I, O)
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
  if (k_splits > 1) {
    const int quads = (int)((long long)n * O / 4);
    hipLaunchKernelGGL(skinny_gemm_bf16_combine_kernel,
                       dim3((quads + 255) / 256), dim3(256), 0, stream,
                       (const f32x4*)partials, (unsigned short*)Y, quads,
                       k_splits);
  }
}
