// Multi-token verify attention for CDNA4/gfx950 (speculative decoding):
// T = 2..8 new tokens per sequence over the slot KV cache, the contract of
// attn_append_ref with Sq = q_lens = T.  Q [n, T, Hq, 128] is already roped
// and the T new K/V rows are already in the cache at
// [slot, q_start : q_start + T); token t attends cache rows kv <= q_start + t.
//
// The kernel grows out of the grouped split-KV decode kernel
// (attention_decode_gqa.hip): grid (splits, Hkv, n), four independent waves
// per block that take the 32-row strips w, w+4, ... of the split's range
// [sp*R, min((sp+1)*R, q_start + T)), K A-fragments straight from global
// memory, V once through wave-private LDS, P^T reused in registers as the B
// fragment, loads one strip ahead (attn_gqa_strip.h holds the shared
// pieces).  What is new:
//
//  * Columns.  The MFMA N dimension holds C = T * group columns, one per
//    (token, q head of the group), in NB = 1 or 2 blocks of 16 columns
//    (template parameter; C <= 32).  The order is token-major,
//    c = t * group + g: the group's heads of one token are adjacent
//    256-byte rows of Q and of O, so consecutive columns are consecutive
//    memory within a token and the epilogue's 16 threads per column write
//    runs of group * 256 contiguous bytes; head-major would stride every
//    column by Hq * 256 bytes.  It also makes the row limit of a column
//    monotone in c.  Columns >= C are zero and are never stored.
//  * Two column blocks share every K fragment and every V fragment read:
//    per strip 8 global K fragments and 8 LDS V fragments feed 16 + 16
//    MFMAs.  The O^T accumulators double (2 x 8 f32x4), so do m, l and the
//    score registers.  With both strip register sets that is more than the
//    256 VGPRs of two waves per SIMD, so for NB = 2 Q^T leaves the registers:
//    it sits in 8 KB of LDS in fragment order and each strip reads its
//    eight fragments back (NB = 1 keeps its four in registers).  The V
//    rows of a strip are staged before the next strip's loads are issued,
//    so the two register sets overlap in K only.  The waves meet in LDS
//    once per column block, through the same [16 q][132] fp32 tile.
//  * Causal mask per column: column c sees rows < lim(c) = q_start + t + 1.
//    Only strips that reach past row q_start can hold a masked score; the
//    test is a scalar (wave-uniform) one and every other strip runs the
//    unmasked path.  The same test covers the ragged last strip, since
//    lim(c) <= q_start + T.  A masked score is -inf before the row maximum
//    and exp2(-inf - m) = +0 exactly, in l and in P.
//  * A column can see no row of a strip, or of a whole split when the T
//    rows straddle a split edge.  Its running maximum is then -inf: the
//    exponent is taken against 0 instead (exp2(-inf - 0) = 0, never
//    inf - inf), the correction of an empty history is 0, and the split
//    hands (m, l, O) = (-inf, 0, 0) to the combine, whose weight
//    exp2(-inf - gm) is 0 (row 0 is visible to every column, so the global
//    maximum gm is finite).
//  * Rows at or past q_start + T are indexed min(row, end - 1) and their V
//    is staged as zeros, as in the decode kernel: no address at or past the
//    range end is formed.
//
// The FP8 KV cache is not served by this kernel.
#include "attn_verify.h"
#include "attn_gqa_strip.h"

// One strip for NB column blocks, its V already staged in `vt`: S^T = K Q^T,
// per-column mask, online softmax, O^T += V^T P^T.  lim[nb] is the lane's column's row limit.
template <int NB>
__device__ __forceinline__ void verify_step(
    const GqaStripBf16& st, int base, bool masked, const int* lim,
    const s16x8* q_b, const s16x8* q_lds, float qscale, float* m, float* l,
    f32x4 (*o)[8], char* vt, int lane) {
  const int kb = lane >> 4, lr = lane & 15;
  // The LDS reads of Q^T are loop-invariant; left to itself the compiler
  // hoists all eight fragments back into registers (and spills).  An
  // opaque copy of the index keeps them in the strip.
  int ql = lane;
  if constexpr (NB > 1) asm volatile("" : "+v"(ql));
  // ---- S^T: 32 kv rows x 16 NB columns; a K fragment serves every block.
  f32x4 acc[NB][2];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
    acc[nb][0] = acc[nb][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      // one block: Q^T lives in registers; two: in LDS, fragment order
      const s16x8 qf = (NB == 1) ? q_b[ks] : q_lds[(4 * nb + ks) * 64 + ql];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
        acc[nb][mb] = MFMA_BF16(as_bf16x8(st.kfrag(4 * mb + ks)),
                                as_bf16x8(qf), acc[nb][mb]);
    }
  s16x8 p_b[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    float s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = acc[nb][i >> 2][i & 3] * qscale;
    if (masked) {  // scalar branch: strips below q_start + 1 skip it
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (base + 16 * (i >> 2) + 4 * kb + (i & 3) >= lim[nb])
          s[i] = -INFINITY;
    }
    float mx = s[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) mx = fmaxf(mx, s[i]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m[nb], mx);
    // a column that has seen no row yet keeps m = -inf and subtracts 0
    const float ms = (mn == -INFINITY) ? 0.f : mn;
    const float corr = (m[nb] == -INFINITY) ? 0.f : gqa_exp2(m[nb] - ms);
    m[nb] = mn;
    float ls = l[nb] * corr;
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[nb][ct][r] *= corr;
    // ---- P^T: the score registers are the B fragment; l sums the
    // unrounded weights.
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float e = gqa_exp2(s[i] - ms);
      ls += e;
      p_b[nb][i] = (short)f2bf(e);
    }
    l[nb] = ls;
  }
  // ---- O^T += V^T P^T, d rows 16ct + lr; a V fragment serves every block.
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) {
    const s16x8 a = gqa_v_frag(vt, ct, kb, lr);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      o[nb][ct] = MFMA_BF16(as_bf16x8(a), as_bf16x8(p_b[nb]), o[nb][ct]);
  }
}

template <int NB>
__global__ __launch_bounds__(256, 2) void attn_verify_kernel(
    const unsigned short* __restrict__ Q,   // [n, T, Hq, 128] roped
    const unsigned short* __restrict__ Kc,  // [slots, S_max, Hkv, 128]
    const unsigned short* __restrict__ Vc,
    unsigned short* __restrict__ O,         // [n, T, Hq, 128]
    float* __restrict__ Ow,                 // [n, T, Hq, splits, 128]
    float* __restrict__ MLw,                // [n, T, Hq, splits, 2]
    const int* __restrict__ slot_ids,       // [n] -> cache slot
    const int* __restrict__ q_start,        // [n] rows before the T tokens
    int T, int S_max, int Hq, int Hkv, int R, float qscale) {
  __shared__ __attribute__((aligned(16))) float lds[4][GQA_WAVE_FLOATS];
  __shared__ float red_m[4][16], red_l[4][16];
  __shared__ s16x8 q_lds[NB > 1 ? NB * 4 * 64 : 1];

  const int sp = blockIdx.x;
  const int kvh = blockIdx.y;
  const int bq = blockIdx.z;
  const int splits = gridDim.x;
  const int group = Hq / Hkv;
  const int C = T * group;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int kb = lane >> 4;
  const int lr = lane & 15;

  // Per-sequence scalars (SGPRs).
  const int slot = __builtin_amdgcn_readfirstlane(slot_ids[bq]);
  const int qs = max(__builtin_amdgcn_readfirstlane(q_start[bq]), 0);
  const int end = min(qs + T, S_max);
  const int r0 = sp * R;
  if (sp > 0 && r0 >= end) return;  // empty split: writes nothing
  const int r1 = min(r0 + R, end);

  // ---- Q^T as B fragments: lane holds q[column 16nb + lr][d = 32ks + 8kb
  // + j] of token c / group, head kvh * group + c % group.
  // One column block keeps them in registers.  Two blocks keep them in
  // LDS in fragment order, [4nb + ks][lane] x 16 bytes (conflict-free, 8
  // KB for the block): wave w loads and writes the fragments ks = w, and
  // every wave reads all eight back per strip.
  s16x8 q_b[4];
  int lim[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int c = 16 * nb + lr;
    const int t = c / group;
    lim[nb] = min(qs + t + 1, end);  // columns >= C: end
    const unsigned short* src =
        Q + (((long long)bq * T + t) * Hq + kvh * group + (c - t * group)) *
                GQA_D + 8 * kb;
    const s16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (NB == 1) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        q_b[ks] = (c < C) ? *(const s16x8*)(src + 32 * ks) : zero;
    } else {
      q_lds[(4 * nb + w) * 64 + lane] =
          (c < C) ? *(const s16x8*)(src + 32 * w) : zero;
    }
  }
  if constexpr (NB > 1) __syncthreads();

  const long long slot_row0 = (long long)slot * S_max * Hkv + kvh;
  const long long rs = (long long)Hkv * GQA_D;  // elements per cache row
  const unsigned short* Kb = Kc + slot_row0 * GQA_D;
  const unsigned short* Vb = Vc + slot_row0 * GQA_D;

  // Softmax state of column 16nb + lr in log2 units; l is the lane's share
  // of the sum.  O^T: o[nb][ct][r] = O[column][d = 16ct + 4kb + r].
  float m[NB], l[NB];
  f32x4 o[NB][8];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    m[nb] = -INFINITY;
    l[nb] = 0.f;
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) o[nb][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  char* vt = (char*)lds[w];

  // ---- the row loop: strips w, w+4, ... of [r0, r1), loads one strip
  // ahead in the other register set.  A strip whose last row is at most
  // q_start holds no masked score.
#define VERIFY_LOAD(st, s) \
  (st).load(Kb, Vb, rs, r0 + GQA_STRIP_ROWS * (s), r1, lane)
#define VERIFY_STEP(st, s)                                               \
  verify_step<NB>(st, r0 + GQA_STRIP_ROWS * (s),                         \
                  r0 + GQA_STRIP_ROWS * ((s) + 1) > qs + 1, lim, q_b,    \
                  q_lds, qscale, m, l, o, vt, lane)
  const int nstrips = (r1 - r0 + GQA_STRIP_ROWS - 1) / GQA_STRIP_ROWS;
  if (w < nstrips) {
    GqaStripBf16 sa, sb;
    int s = w;
    VERIFY_LOAD(sa, s);
    for (;;) {
      bool last = s + 4 >= nstrips;
      gqa_stage_v(sa, vt, kb, lr);
      VERIFY_LOAD(sb, last ? s : s + 4);
      VERIFY_STEP(sa, s);
      if (last) break;
      s += 4;
      last = s + 4 >= nstrips;
      gqa_stage_v(sb, vt, kb, lr);
      VERIFY_LOAD(sa, last ? s : s + 4);
      VERIFY_STEP(sb, s);
      if (last) break;
      s += 4;
    }
  }
#undef VERIFY_LOAD
#undef VERIFY_STEP

  // ---- the four waves meet in LDS, one column block at a time: O^T
  // partial as [q][d], m and l.  Thread (col, c8) merges column col.
  const int col = tid >> 4;  // column of the block
  const int c8 = tid & 15;   // d = 8 c8 .. 8 c8 + 7
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (nb > 0) __syncthreads();  // the readers of the block before
    float lw = l[nb];
    lw += __shfl_xor(lw, 16, 64);
    lw += __shfl_xor(lw, 32, 64);
    float* ow = lds[w];
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
      *(f32x4*)(ow + lr * GQA_O_STRIDE + 16 * ct + 4 * kb) = o[nb][ct];
    if (kb == 0) {
      red_m[w][lr] = m[nb];
      red_l[w][lr] = lw;
    }
    __syncthreads();
    const int c = 16 * nb + col;
    if (c >= C) continue;
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
      const float* src = lds[i] + col * GQA_O_STRIDE + 8 * c8;
      const f32x4 x0 = *(const f32x4*)src;
      const f32x4 x1 = *(const f32x4*)(src + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[j] += x0[j] * cc;
        a[j + 4] += x1[j] * cc;
      }
    }
    const int t = c / group;
    const long long row =
        ((long long)bq * T + t) * Hq + kvh * group + (c - t * group);
    if (splits == 1) {
      const float inv = (gl > 0.f) ? 1.f / gl : 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] *= inv;
      *(s16x8*)(O + row * GQA_D + 8 * c8) = f32_to_bf8(a);
      continue;
    }
    float* dstp = Ow + (row * splits + sp) * GQA_D + 8 * c8;
    *(f32x4*)dstp = f32x4{a[0], a[1], a[2], a[3]};
    *(f32x4*)(dstp + 4) = f32x4{a[4], a[5], a[6], a[7]};
    if (c8 == 0) {
      MLw[(row * splits + sp) * 2] = gm;
      MLw[(row * splits + sp) * 2 + 1] = gl;
    }
  }
}

// Merge of the splits: one wave per (sequence, token, q head), two d per
// lane.  attn_decode_combine_kernel takes its split count from a kv_lens
// [n] tensor that the verify step does not have; this variant reads
// q_start, so no launch is spent on building one.  Only splits
// sp < ceil((q_start + T) / R) were written; a split in which the row saw
// nothing holds m = -inf, l = 0, O = 0 and gets weight 0.
extern "C" __global__ __launch_bounds__(256) void attn_verify_combine_kernel(
    const float* __restrict__ Ow,    // [n*T*Hq, splits, 128]
    const float* __restrict__ MLw,   // [n*T*Hq, splits, 2]
    unsigned short* __restrict__ O,  // [n*T*Hq, 128]
    const int* __restrict__ q_start, int total, int T, int Hq, int S_max,
    int splits, int R) {
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= total) return;
  const int end = min(max(q_start[idx / (T * Hq)], 0) + T, S_max);
  const int nsp = min(max(1, (end + R - 1) / R), splits);
  const float* ml = MLw + (long long)idx * splits * 2;
  float gm = -INFINITY;
  for (int sp = 0; sp < nsp; ++sp) gm = fmaxf(gm, ml[2 * sp]);
  const float* ow = Ow + (long long)idx * splits * GQA_D + 2 * lane;
  float gl = 0.f, a0 = 0.f, a1 = 0.f;
  for (int sp = 0; sp < nsp; ++sp) {
    const float cc = gqa_exp2(ml[2 * sp] - gm);  // exp2(-inf) = 0
    gl += ml[2 * sp + 1] * cc;
    const f32x2 v = *(const f32x2*)(ow + sp * GQA_D);
    a0 += v[0] * cc;
    a1 += v[1] * cc;
  }
  const float inv = (gl > 0.f) ? 1.f / gl : 0.f;
  s16x2 out = {(short)f2bf(a0 * inv), (short)f2bf(a1 * inv)};
  *(s16x2*)(O + (long long)idx * GQA_D + 2 * lane) = out;
}

static const float kLog2e = 1.44269504088896340736f;

extern "C" void attn_verify_launch(const void* Q, const void* Kc,
                                   const void* Vc, void* O, void* Ow,
                                   void* MLw, const int* slot_ids,
                                   const int* q_start, int n, int T,
                                   int S_max, int Hq, int Hkv, int split_rows,
                                   int splits, float scale,
                                   hipStream_t stream) {
  const dim3 grid(splits, Hkv, n), block(256);
  auto* kernel = (T * (Hq / Hkv) <= 16) ? attn_verify_kernel<1>
                                        : attn_verify_kernel<2>;
  hipLaunchKernelGGL(kernel, grid, block, 0, stream,
                     (const unsigned short*)Q, (const unsigned short*)Kc,
                     (const unsigned short*)Vc, (unsigned short*)O,
                     (float*)Ow, (float*)MLw, slot_ids, q_start, T, S_max, Hq,
                     Hkv, split_rows, scale * kLog2e);
  if (splits > 1) {
    const int total = n * T * Hq;
    hipLaunchKernelGGL(attn_verify_combine_kernel, dim3((total + 3) / 4),
                       dim3(256), 0, stream, (const float*)Ow,
                       (const float*)MLw, (unsigned short*)O, q_start, total,
                       T, Hq, S_max, splits, split_rows);
  }
}
