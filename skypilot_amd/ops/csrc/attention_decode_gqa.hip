// Grouped split-KV decode attention for CDNA4/gfx950: the contract of
// attn_decode_qkv / attn_decode_qkv_fp8 (attention_decode.hip,
// attention_decode_fp8.hip) with one block per (sequence, KV head, kv
// range) instead of one per (sequence, q head).
//
// The q heads of a GQA group are the N dimension of a 16x16x32 MFMA, so a
// K/V row is read once for the whole group, and the kv length is split
// across blocks (grid (splits, Hkv, n)); attn_decode_combine_kernel merges
// the splits.  Split sp owns cache rows [sp*R, min((sp+1)*R, p)), R fixed
// by the host from S_max alone (attn_decode_gqa.h), so a sequence's output
// bits do not depend on the batch it rides in.
//
// Inside a block the four waves are independent: wave w takes the 32-row
// strips w, w+4, ... of the range with its own online softmax and its own
// O^T accumulators, and the waves meet once, at the end, in LDS.  No
// __syncthreads in the row loop.
//
//  * S^T = K Q^T.  Q^T is the B operand (column l&15 = q head of the
//    group, columns >= group zero), roped in fp32 and rounded once to
//    bf16.  K A-fragments come straight from global memory: lane
//    (kb, row) = (l>>4, l&15) loads 16 bytes (fp8: 8) of K row `row` at
//    d = 32ks + 8kb.  K never touches LDS.  scale * log2(e) multiplies the
//    fp32 scores.
//  * The lane's eight score registers of the strip's two M-blocks are
//    strip rows 16mb + 4kb + r.  The contraction index of O^T = V^T P^T
//    may be any permutation of the strip's rows as long as V uses the
//    same one: k-slot 8kb + j is strip row 16(j>>2) + 4kb + (j&3), and the
//    eight registers, after exp2 and one bf16 pack, ARE the lane's B
//    fragment.  No shuffle.
//  * V crosses LDS once, wave-private: lane (kb, c) loads chunk c of rows
//    16mb + 4kb + r, packs the four rows of one d into 8 bytes (k-slots
//    8kb + 4mb ..+3) and writes them with ds_write_b64 into a [d][k-slot]
//    tile whose d rows are stored at (d&7)*16 + (d>>3); the A fragments
//    come back as ds_read_b128.
//  * Loads run one strip ahead in a second register set; the last
//    iteration re-reads its own strip, so the loop has one shape.
//  * Rows of a strip at or past the range end are indexed min(row, end-1)
//    and their score is masked; their V is staged as zeros (0 * NaN).  A
//    strip wholly below the end takes plain loads (wave-uniform test).  No
//    address at or past row p of the slot is formed by a reader.
//  * Split 0, wave 0 attends the current token from registers (l = 1,
//    O^T = v) and writes row p for later steps; fp8 quantises it with
//    kv_fp8.h and attends code * 2^n.
//
// The kernel body (attn_decode_gqa_body.h) is included once per K/V source.
#include "attn_decode_gqa.h"
#include "attn_gqa_strip.h"
#include "kv_fp8.h"

// FP8 cache (kv_fp8.h): 8-byte chunks of codes, and the exponent bytes of
// the lane's eight score rows 16mb + 4(l>>4) + r, which are also its V
// rows.  The fragments are the unscaled codes as bf16 (exact); the K scale
// multiplies the fp32 score and the V scale the weight, both powers of two.
struct GqaStripFp8 {
  i32x2 k[8], v[8];
  unsigned ke[8], ve[8];  // [4mb + r]
  __device__ __forceinline__ void load(const unsigned char* Kb,
                                       const unsigned char* Vb,
                                       const unsigned char* Keb,
                                       const unsigned char* Veb,
                                       long long rs, int Hkv, int base,
                                       int end, int lane) {
    const int kb = lane >> 4, lr = lane & 15;
    const bool full = base + GQA_STRIP_ROWS <= end;  // wave-uniform
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int krow = base + 16 * mb + lr;
      const unsigned char* kr =
          Kb + (long long)(full ? krow : min(krow, end - 1)) * rs + 8 * kb;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        k[4 * mb + ks] = *(const i32x2*)(kr + 32 * ks);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int vrow = base + 16 * mb + 4 * kb + r;
        // never past the valid rows, codes and exponents alike
        const long long rc = full ? vrow : min(vrow, end - 1);
        const i32x2 vv = *(const i32x2*)(Vb + rc * rs + 8 * lr);
        // code 0 is +0
        v[4 * mb + r] = (full || vrow < end) ? vv : i32x2{0, 0};
        ke[4 * mb + r] = Keb[rc * Hkv];
        ve[4 * mb + r] = Veb[rc * Hkv];
      }
    }
  }
  __device__ __forceinline__ s16x8 kfrag(int i) const {
    return kv8_dequant_bf16(k[i], 1.f);
  }
  __device__ __forceinline__ s16x8 vrow(int i) const {
    return kv8_dequant_bf16(v[i], 1.f);
  }
};

// One strip: stage V, S^T = K Q^T, online softmax, O^T += V^T P^T.
template <bool FP8, class Strip>
__device__ __forceinline__ void gqa_step(const Strip& st, int base, int end,
                                         const s16x8* q_b, float qscale,
                                         float& m, float& l, f32x4* o,
                                         char* vt, int lane) {
  const int kb = lane >> 4, lr = lane & 15;
  gqa_stage_v(st, vt, kb, lr);
  // ---- S^T: 32 kv rows x 16 q heads.
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
      acc[mb] = MFMA_BF16(as_bf16x8(st.kfrag(4 * mb + ks)),
                          as_bf16x8(q_b[ks]), acc[mb]);
  const bool full = base + GQA_STRIP_ROWS <= end;  // wave-uniform
  float s[8];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float x = acc[i >> 2][i & 3];
    if constexpr (FP8) x *= kv8_scale(st.ke[i]);
    x *= qscale;
    if (!full && base + 16 * (i >> 2) + 4 * kb + (i & 3) >= end)
      x = -INFINITY;
    s[i] = x;
    mx = fmaxf(mx, x);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  // every strip has a row below `end`, so mn is finite
  const float mn = fmaxf(m, mx);
  const float corr = (m == -INFINITY) ? 0.f : gqa_exp2(m - mn);
  m = mn;
  l *= corr;
#pragma unroll
  for (int ct = 0; ct < 8; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) o[ct][r] *= corr;
  // ---- P^T: the score registers are the B fragment; l sums the
  // unrounded weights (per lane, the four lane groups are added at the end).
  s16x8 p_b;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float e = gqa_exp2(s[i] - mn);
    l += e;
    if constexpr (FP8) e *= kv8_scale(st.ve[i]);
    p_b[i] = (short)f2bf(e);
  }
  // ---- O^T += V^T P^T, d rows 16ct + lr.
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) {
    const s16x8 a = gqa_v_frag(vt, ct, kb, lr);
    o[ct] = MFMA_BF16(as_bf16x8(a), as_bf16x8(p_b), o[ct]);
  }
}

// Rope of the 8 elements [8c, 8c+8) of a head (the row layout of
// kv_fp8.h): own chunk and the chunk 64 elements away.
__device__ __forceinline__ void gqa_rope8(const unsigned short* head, int c,
                                          const float* cs, const float* sn,
                                          float* out) {
  float own[8], par[8];
  bf8_to_f32(*(const s16x8*)(head + c * 8), own);
  bf8_to_f32(*(const s16x8*)(head + (c ^ 8) * 8), par);
  const float sgn = (c < 8) ? -1.f : 1.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = own[j] * cs[j] + sgn * par[j] * sn[j];
}

#define GQA_KERNEL attn_decode_gqa_kernel
#define GQA_FP8 0
#include "attn_decode_gqa_body.h"
#undef GQA_KERNEL
#undef GQA_FP8

#define GQA_KERNEL attn_decode_gqa_fp8_kernel
#define GQA_FP8 1
#include "attn_decode_gqa_body.h"
#undef GQA_KERNEL
#undef GQA_FP8

// Merge of the splits: one wave per (sequence, q head), two d per lane.
// Only splits sp < max(1, ceil(p / R)) were written.
extern "C" __global__ __launch_bounds__(256) void attn_decode_combine_kernel(
    const float* __restrict__ Ow,   // [n*Hq, splits, 128]
    const float* __restrict__ MLw,  // [n*Hq, splits, 2]
    unsigned short* __restrict__ O, // [n*Hq, 128]
    const int* __restrict__ kv_lens, int total, int Hq, int splits, int R) {
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= total) return;
  const int nc = max(kv_lens[idx / Hq] - 1, 0);
  const int nsp = min(max(1, (nc + R - 1) / R), splits);
  const float* ml = MLw + (long long)idx * splits * 2;
  float gm = -INFINITY;
  for (int sp = 0; sp < nsp; ++sp) gm = fmaxf(gm, ml[2 * sp]);
  const float* ow = Ow + (long long)idx * splits * GQA_D + 2 * lane;
  float gl = 0.f, a0 = 0.f, a1 = 0.f;
  for (int sp = 0; sp < nsp; ++sp) {
    const float cc = gqa_exp2(ml[2 * sp] - gm);
    gl += ml[2 * sp + 1] * cc;
    const f32x2 v = *(const f32x2*)(ow + sp * GQA_D);
    a0 += v[0] * cc;
    a1 += v[1] * cc;
  }
  const float inv = (gl > 0.f) ? 1.f / gl : 0.f;
  s16x2 out = {(short)f2bf(a0 * inv), (short)f2bf(a1 * inv)};
  *(s16x2*)(O + (long long)idx * GQA_D + 2 * lane) = out;
}

static void gqa_combine(void* O, const void* Ow, const void* MLw,
                        const int* kv_lens, int n, int Hq, int R, int splits,
                        hipStream_t stream) {
  const int total = n * Hq;
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3((total + 3) / 4),
                     dim3(256), 0, stream, (const float*)Ow,
                     (const float*)MLw, (unsigned short*)O, kv_lens, total,
                     Hq, splits, R);
}

static const float kLog2e = 1.44269504088896340736f;

extern "C" void attn_decode_gqa_launch(
    const void* qkv, void* Kc, void* Vc, void* O, void* Ow, void* MLw,
    const void* cos_tab, const void* sin_tab, const int* positions,
    const int* kv_lens, const int* slot_ids, int n, int S_max, int Hq,
    int Hkv, int split_rows, int splits, float scale, hipStream_t stream) {
  hipLaunchKernelGGL(attn_decode_gqa_kernel, dim3(splits, Hkv, n), dim3(256),
                     0, stream, (const unsigned short*)qkv,
                     (unsigned short*)Kc, (unsigned short*)Vc,
                     (unsigned short*)O, (float*)Ow, (float*)MLw,
                     (const float*)cos_tab, (const float*)sin_tab, positions,
                     kv_lens, slot_ids, S_max, Hq, Hkv, split_rows,
                     scale * kLog2e);
  if (splits > 1)
    gqa_combine(O, Ow, MLw, kv_lens, n, Hq, split_rows, splits, stream);
}

extern "C" void attn_decode_gqa_fp8_launch(
    const void* qkv, void* Kc, void* Vc, void* Ke, void* Ve, void* O,
    void* Ow, void* MLw, const void* cos_tab, const void* sin_tab,
    const int* positions, const int* kv_lens, const int* slot_ids, int n,
    int S_max, int Hq, int Hkv, int split_rows, int splits, float scale,
    hipStream_t stream) {
  hipLaunchKernelGGL(attn_decode_gqa_fp8_kernel, dim3(splits, Hkv, n),
                     dim3(256), 0, stream, (const unsigned short*)qkv,
                     (unsigned char*)Kc, (unsigned char*)Vc,
                     (unsigned char*)Ke, (unsigned char*)Ve,
                     (unsigned short*)O, (float*)Ow, (float*)MLw,
                     (const float*)cos_tab, (const float*)sin_tab, positions,
                     kv_lens, slot_ids, S_max, Hq, Hkv, split_rows,
                     scale * kLog2e);
  if (splits > 1)
    gqa_combine(O, Ow, MLw, kv_lens, n, Hq, split_rows, splits, stream);
}
