// Presence, frequency and repetition penalties for the decode step: one
// row of bf16 logits and the token history of its sequence in, one
// penalised row out, one workgroup per row.  The definition
// (docs/KERNELS.md "Decode penalties") is shared with
// ops.penalize_logits_reference; this file is its GPU form.
//
// Design, in the order the row is processed:
//
//   1. copy     the row goes to `out` with the sampler's traversal: each
//               wave owns a contiguous segment and moves it with 16-byte
//               loads and stores, four loads in flight per lane.  Rows
//               that are off (no penalty set, or an index outside the
//               history) stop here: the history is neither read nor
//               written.
//   2. count    thread i of the history walk records the input token at
//               hist[s, p] and adds position i's token into the row's
//               count workspace cnt[row, id] with ONE integer atomic:
//               +1 for a generated position (i >= P), +0x10000 for a
//               prompt position.  No sort, no LDS table, so no capacity
//               limit; the walk touches only the tokens the sequence has
//               seen.
//   3. apply    after one barrier the same walk exchanges every visited
//               word with 0.  Exactly one thread per distinct token gets
//               the non-zero word; it computes the penalised value from
//               the INPUT logit and the generated count and overwrites
//               the copied element with a 2-byte store.
//
// The exchange of step 3 leaves cnt all zero again, which is the
// invariant the workspace is allocated with: there is no clearing pass
// and no V-sized traffic beyond the copy.  Counts are integers and the
// value is a function of the count alone, so the result does not depend
// on which thread wins a word: the row is a pure function of its inputs
// and TP ranks agree without communication.
//
// The barrier between 2 and 3 also orders the copy's store to an element
// before the apply's store to it (__syncthreads is a workgroup-scope
// release/acquire fence around the barrier).
//
// Both counts share a 32-bit word, 16 bits each: the binding bounds S_max
// by 65535.  Every loop is bounded by V or by p + 1 <= S_max.  The index
// tensors are read on the device (no host sync; graph-capturable); the
// atomics are ordinary device-scope HIP atomics issued per lane, every
// store is a plain vector store.
#include "common.h"
#include "row_pass.h"

#define PENALTY_THREADS 1024
#define PENALTY_PROMPT_ONE 0x10000u  // a prompt occurrence in a count word

// The penalised value of a seen token (docs/KERNELS.md): repetition on
// the raw logit, then frequency and presence on the generated count, in
// fp32, rounded to bf16 (nearest even).  -inf stays -inf, NaN stays NaN.
__device__ __forceinline__ unsigned short penalised(unsigned short h,
                                                    unsigned c, float alpha,
                                                    float beta, float rho) {
  float x = bf2f(h);
  if (rho != 1.f) x = x > 0.f ? x / rho : x * rho;
  x = x - beta * (float)c - (c > 0u ? alpha : 0.f);
  return f2bf(x);
}

template <int NT>
__global__ __launch_bounds__(NT) void penalize_logits_kernel(
    const unsigned short* __restrict__ logits,  // [n, V]
    unsigned short* __restrict__ out,           // [n, V]
    int V,
    int* __restrict__ hist,                     // [slots, S_max]
    int slots, int S_max,
    unsigned* __restrict__ cnt,                 // [>= n, V], all zero
    const int* __restrict__ tok, const int* __restrict__ pos,
    const int* __restrict__ slot, const int* __restrict__ prompt_len,
    const float* __restrict__ presence, const float* __restrict__ frequency,
    const float* __restrict__ repetition) {
  constexpr int NW = NT / WAVE;
  const long long i = blockIdx.x;
  const unsigned short* __restrict__ row = logits + i * V;
  unsigned short* __restrict__ orow = out + i * V;

  // ---- 1. copy ----------------------------------------------------------
  {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    // per-wave segment: a multiple of 4 steps of 512 elements
    const int seg =
        (int)((((long long)V + NW - 1) / NW + 2047) / 2048 * 2048);
    const int iters = seg / 512;
    const int base = wid * seg + lane * 8;
    const bool in_ok = ((unsigned long long)row & 15ull) == 0;
    const bool out_ok = ((unsigned long long)orow & 15ull) == 0;
    for (int it0 = 0; it0 < iters; it0 += 4) {
      s16x8 x[4];
#pragma unroll
      for (int g = 0; g < 4; ++g)
        x[g] = load8(row, V, in_ok, base + (it0 + g) * 512);
#pragma unroll
      for (int g = 0; g < 4; ++g)
        store8(orow, V, out_ok, base + (it0 + g) * 512, x[g]);
    }
  }

  const float alpha = presence[i];
  const float beta = frequency[i];
  const float rho = repetition[i];
  const int s = slot[i];
  const int p = pos[i];
  // off rows and rows whose index would leave hist: uniform over the block
  if (alpha == 0.f && beta == 0.f && rho == 1.f) return;
  if (s < 0 || s >= slots || p < 0 || p >= S_max) return;
  const int t = tok[i];
  int P = prompt_len[i];
  P = P < 0 ? 0 : (P > p + 1 ? p + 1 : P);
  int* h = hist + (long long)s * S_max;
  unsigned* c = cnt + i * V;

  // ---- 2. record and count ------------------------------------------------
  // Position p is the input token itself: its thread stores it and uses
  // the value it holds, so no thread reads hist[s, p] in this launch.
  for (int j = threadIdx.x; j <= p; j += NT) {
    int id;
    if (j == p) {
      id = t;
      h[j] = t;
    } else {
      id = h[j];
    }
    if (id >= 0 && id < V)
      atomicAdd(&c[id], j >= P ? 1u : PENALTY_PROMPT_ONE);
  }
  __syncthreads();

  // ---- 3. claim and apply ---------------------------------------------------
  for (int j = threadIdx.x; j <= p; j += NT) {
    const int id = j == p ? t : h[j];
    if (id >= 0 && id < V) {
      const unsigned w = atomicExch(&c[id], 0u);
      if (w != 0u)
        orow[id] = penalised(row[id], w & 0xffffu, alpha, beta, rho);
    }
  }
}

extern "C" void penalize_logits_launch(
    const void* logits, void* out, int V, long long n, void* hist, int slots,
    int S_max, void* cnt, const void* tok, const void* pos, const void* slot,
    const void* prompt_len, const void* presence, const void* frequency,
    const void* repetition, hipStream_t stream) {
  hipLaunchKernelGGL(penalize_logits_kernel<PENALTY_THREADS>,
                     dim3((unsigned)n), dim3(PENALTY_THREADS), 0, stream,
                     (const unsigned short*)logits, (unsigned short*)out, V,
                     (int*)hist, slots, S_max, (unsigned*)cnt,
                     (const int*)tok, (const int*)pos, (const int*)slot,
                     (const int*)prompt_len, (const float*)presence,
                     (const float*)frequency, (const float*)repetition);
}
