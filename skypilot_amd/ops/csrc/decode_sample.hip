// Seeded in-graph sampling for the decode step: temperature, top-k and
// top-p over one row of bf16 logits, one workgroup per row.  The
// definition (docs/KERNELS.md "Decode sampling") is shared with
// ops.sample_tokens_reference; this file is its GPU form.
//
// Design, in the order the row is processed:
//
//   1. argmax pass       max value m and its lowest index (also the
//                        answer for T == 0 and for degenerate rows);
//   2. threshold search  a two-level 256-bin radix walk over an order-
//                        preserving 16-bit key of the bf16 value: one
//                        pass histograms count and mass by the key's
//                        high byte (its total is Z), a second by the low
//                        byte inside the chosen bin (skipped when no
//                        filter is on);
//   3. draw              kept mass per wave, then one wave walks its
//                        segment in index order to the first prefix sum
//                        above u * Z_K.
//
// Every weight is turned into a 64-bit fixed-point integer
// (floor(w * 2^40), w in [0, 1]) before it is summed.  Integer sums are
// exact and associative, so every total is independent of the order it
// was formed in: the result is a pure function of the inputs (no
// floating-point reduction order to pin down, no floating-point
// atomics; the histograms use integer LDS atomics, whose order cannot
// matter), a partial sum found at one level of the draw or of the
// radix walk is found again one level down, and the mass at or above
// the lowest key is exactly Z.  The price is a truncation error of at
// most V * 2^-40 of the (>= 1) total, far below the fp32 rounding of
// any float accumulation.
// A row's total is at most V * 2^40, so the bindings bound V at 2^23:
// no sum can wrap 64 bits.
//
// Each wave owns a contiguous segment of the row and reads it with
// 16-byte loads, four in flight per lane; the 256 KB row of a 128k
// vocabulary stays in L2 across the passes.  All loops are bounded by V
// or by the 256 bins.  State writes are plain vector stores from
// thread 0.
#include "common.h"

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

// Word 0 of Philox4x32-10 with counter (c0, 0, 0, 0), key (k0, k1).
__host__ __device__ __forceinline__ void philox4x32_10(unsigned c[4],
                                                       unsigned k0,
                                                       unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += PHILOX_W0;
      k1 += PHILOX_W1;
    }
    const unsigned long long p0 = (unsigned long long)PHILOX_M0 * c[0];
    const unsigned long long p1 = (unsigned long long)PHILOX_M1 * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = (unsigned)p1;
    c[2] = n2;
    c[3] = (unsigned)p0;
  }
}

typedef unsigned long long u64;

// Order-preserving 16-bit key of a bf16 value; -0 maps to +0's key so
// equal values share a key.  NaN rows never reach the key search.
__device__ __forceinline__ unsigned bf_key(unsigned short h) {
  if (h == 0x8000u) h = 0;
  return (h & 0x8000u) ? (~(unsigned)h & 0xffffu) : ((unsigned)h | 0x8000u);
}

__device__ __forceinline__ float key_value(unsigned k) {
  const unsigned short h =
      (k & 0x8000u) ? (unsigned short)(k & 0x7fffu)
                    : (unsigned short)(~k & 0xffffu);
  return bf2f(h);
}

// floor(exp((l - m) / T) * 2^40) with scale = log2(e) / T.  The clamp
// sends -inf logits (and a NaN from -inf * 0) to weight 0: v_max
// returns its non-NaN operand.
__device__ __forceinline__ u64 weight_q(float l, float m, float scale) {
  const float a = fmaxf((l - m) * scale, -126.f);
  return (u64)(__builtin_amdgcn_exp2f(a) * 1099511627776.f);
}

__device__ __forceinline__ u64 wave_sum_u64(u64 x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
  return x;
}

#define HR 16  // histogram copies: lane l adds into copy l % HR

template <int NT>
struct SampleSmem {
  u64 wsum[NT / WAVE];
  float wmax[NT / WAVE];
  int widx[NT / WAVE];
  int wnan[NT / WAVE];
  int tok;
  // threshold search: HR copies of 256 bins, their sums, the chosen digit
  unsigned hcnt[256 * HR];
  u64 hmass[256 * HR];
  unsigned bcnt[256];
  u64 bmass[256];
  unsigned sel_digit;
  unsigned sel_cnt;
  u64 sel_mass;
};

// 8 consecutive elements from row[idx..]; positions >= V read as 0.
__device__ __forceinline__ s16x8 load8(const unsigned short* __restrict__ row,
                                       int V, bool vec_ok, int idx) {
  s16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (vec_ok && idx + 8 <= V) {
    v = *(const s16x8*)(row + idx);
  } else if (idx < V) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (idx + k < V) v[k] = (short)row[idx + k];
  }
  return v;
}

// Row traversal shared by every pass.  Wave `wid` owns elements
// [wid * seg, (wid + 1) * seg); in step `it` lane `lane` holds the 8
// elements from wid * seg + it * 512 + lane * 8.  f(idx, h, valid) is
// called for all 8 in index order; !valid marks positions >= V.
template <typename F>
__device__ __forceinline__ void row_pass(const unsigned short* __restrict__ row,
                                         int V, bool vec_ok, int base,
                                         int iters, F f) {
  for (int it0 = 0; it0 < iters; it0 += 4) {
    s16x8 x[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
      x[g] = load8(row, V, vec_ok, base + (it0 + g) * 512);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int idx = base + (it0 + g) * 512;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        f(idx + k, (unsigned short)x[g][k], idx + k < V);
    }
  }
}

struct SampleResult {
  int tok;
  float tau;
};

// Samples one row with the whole block.  Every thread returns the same
// result; tok is always in [0, V).
template <int NT>
__device__ __forceinline__ SampleResult sample_row(const unsigned short* __restrict__ row,
                                   int V, float T, float top_p, int top_k,
                                   unsigned seed_lo, unsigned seed_hi,
                                   unsigned counter, SampleSmem<NT>& sm) {
  constexpr int NW = NT / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  // per-wave segment: a multiple of 4 steps of 512 elements
  const int seg = (int)((((long long)V + NW - 1) / NW + 2047) / 2048 * 2048);
  const int iters = seg / 512;
  const int base = wid * seg + lane * 8;
  const bool vec_ok = ((unsigned long long)row & 15ull) == 0;

  // ---- 1. argmax (lowest index wins ties; NaN never wins) -------------
  float best = -INFINITY;
  int bidx = 0;
  int has_nan = 0;
  row_pass(row, V, vec_ok, base, iters,
           [&](int j, unsigned short h, bool valid) {
             const float v = bf2f(h);
             if (valid && v > best) {
               best = v;
               bidx = j;
             }
             has_nan |= (valid && v != v);
           });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, WAVE);
    const int oi = __shfl_xor(bidx, off, WAVE);
    has_nan |= __shfl_xor(has_nan, off, WAVE);
    if (ov > best || (ov == best && oi < bidx)) {
      best = ov;
      bidx = oi;
    }
  }
  if (lane == 0) {
    sm.wmax[wid] = best;
    sm.widx[wid] = bidx;
    sm.wnan[wid] = has_nan;
  }
  __syncthreads();
  best = sm.wmax[0];
  bidx = sm.widx[0];
  has_nan = sm.wnan[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    const float ov = sm.wmax[w];
    const int oi = sm.widx[w];
    has_nan |= sm.wnan[w];
    if (ov > best || (ov == best && oi < bidx)) {
      best = ov;
      bidx = oi;
    }
  }
  __syncthreads();
  const float m = best;
  SampleResult res;
  res.tok = bidx;
  res.tau = -INFINITY;
  // Greedy rows, and rows whose weights are undefined (NaN present, max
  // +-inf: exactly the rows whose Z is not finite), take the argmax.
  if (!(T > 0.f) || has_nan || !(fabsf(m) < INFINITY)) return res;

  // log2(e) / T, kept finite so that (m - m) * scale is 0 for any T > 0
  const float scale = fminf(1.44269504088896340736f / T, 3.0e38f);
  const bool use_k = top_k > 0 && top_k < V;
  const bool use_p = top_p < 1.f;

  // ---- 2. threshold key: two-level 256-bin radix walk --------------
  // Level 0 histograms the high byte of every key, level 1 the low byte
  // of the keys in the chosen high bin: count (and, for top_p, fixed-
  // point mass) per bin through integer LDS atomics into HR copies of
  // the bins, so that the lanes of a wave spread over the copies.  The
  // filter predicate "count >= top_k or mass >= top_p * Z at or above
  // this digit" is monotone, holds at digit 0 of either level and
  // requires a non-empty set, so exactly one digit d has it while d + 1
  // does not; that digit's thread publishes it.  The key so chosen is a
  // value present in the row: tau.
  unsigned tkey = 0;  // keep everything
  if (use_k || use_p) {
    unsigned prefix = 0;      // digits chosen so far
    unsigned cnt_above = 0;   // totals strictly above the chosen bins
    u64 mass_above = 0;
    double p_mass = 0.0;      // top_p * Z
    const int copy = lane & (HR - 1);
#pragma unroll 1
    for (int level = 0; level < 2; ++level) {
      for (int i = threadIdx.x; i < 256 * HR; i += NT) {
        sm.hcnt[i] = 0u;
        sm.hmass[i] = 0ull;
      }
      __syncthreads();
      const int shift = level == 0 ? 8 : 0;
      row_pass(row, V, vec_ok, base, iters,
               [&](int, unsigned short h, bool valid) {
                 const unsigned key = bf_key(h);
                 if (valid && (level == 0 || (key >> 8) == prefix)) {
                   const unsigned d = (key >> shift) & 255u;
                   atomicAdd(&sm.hcnt[d * HR + copy], 1u);
                   if (use_p)
                     atomicAdd(&sm.hmass[d * HR + copy],
                               weight_q(bf2f(h), m, scale));
                 }
               });
      __syncthreads();
      if (threadIdx.x < 256) {
        unsigned c = 0;
        u64 q = 0;
#pragma unroll
        for (int r = 0; r < HR; ++r) {
          c += sm.hcnt[threadIdx.x * HR + r];
          q += sm.hmass[threadIdx.x * HR + r];
        }
        sm.bcnt[threadIdx.x] = c;
        sm.bmass[threadIdx.x] = q;
      }
      __syncthreads();
      if (threadIdx.x < 256) {
        const int d = threadIdx.x;
        unsigned c0 = cnt_above, c1 = cnt_above;  // at or above d / d + 1
        u64 m0 = mass_above, m1 = mass_above, tot = mass_above;
        for (int e = 255; e >= 0; --e) {
          const unsigned c = sm.bcnt[e];
          const u64 q = sm.bmass[e];
          tot += q;
          if (e >= d) {
            c0 += c;
            m0 += q;
          }
          if (e > d) {
            c1 += c;
            m1 += q;
          }
        }
        if (level == 0) p_mass = (double)fmaxf(top_p, 0.f) * (double)tot;
        auto holds = [&](unsigned c, u64 q) {
          return c >= 1u && ((use_k && c >= (unsigned)top_k) ||
                             (use_p && (double)q >= p_mass));
        };
        if (holds(c0, m0) && !holds(c1, m1)) {
          sm.sel_digit = (unsigned)d;
          sm.sel_cnt = c1;
          sm.sel_mass = m1;
        }
      }
      __syncthreads();
      prefix = (prefix << 8) | sm.sel_digit;
      cnt_above = sm.sel_cnt;
      mass_above = sm.sel_mass;
    }
    tkey = prefix;
    res.tau = key_value(tkey);
  }

  // ---- 3. draw --------------------------------------------------------
  u64 my = 0;
  row_pass(row, V, vec_ok, base, iters,
           [&](int, unsigned short h, bool valid) {
             const bool keep = valid && bf_key(h) >= tkey;
             const u64 q = weight_q(bf2f(h), m, scale);
             my += keep ? q : 0ull;
           });
  my = wave_sum_u64(my);
  if (lane == 0) sm.wsum[wid] = my;
  if (threadIdx.x == 0) sm.tok = bidx;  // the argmax is always kept
  __syncthreads();
  u64 zk = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) zk += sm.wsum[w];
  unsigned c[4] = {counter, 0u, 0u, 0u};
  philox4x32_10(c, seed_lo, seed_hi);
  const u64 r = (u64)(c[0] >> 8);
  // floor(r * zk / 2^24): the first integer prefix sum above u * Z_K is
  // the first one above this, and it exists because u < 1.
  const u64 t = (zk >> 24) * r + (((zk & 0xffffffull) * r) >> 24);
  int wsel = NW - 1;
  u64 pre = 0;
  {
    u64 run = 0;
    bool found = false;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const u64 s = sm.wsum[w];
      if (!found && run + s > t) {
        wsel = w;
        pre = run;
        found = true;
      }
      run += s;
    }
  }
  if (wid == wsel) {
    bool done = false;
    for (int it = 0; it < iters && !done; ++it) {
      const int idx = base + it * 512;
      const s16x8 x = load8(row, V, vec_ok, idx);
      u64 q[8];
      u64 ls = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const unsigned short h = (unsigned short)x[k];
        const bool keep = idx + k < V && bf_key(h) >= tkey;
        q[k] = keep ? weight_q(bf2f(h), m, scale) : 0ull;
        ls += q[k];
      }
      u64 incl = ls;
#pragma unroll
      for (int off = 1; off < WAVE; off <<= 1) {
        const u64 o = __shfl_up(incl, off, WAVE);
        if (lane >= off) incl += o;
      }
      const u64 tot = __shfl(incl, WAVE - 1, WAVE);
      if (pre + tot > t) {
        const unsigned long long hit = __ballot(pre + incl > t);
        const int first = __ffsll((long long)hit) - 1;
        if (lane == first) {
          u64 run = pre + incl - ls;
          int tok = -1;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            run += q[k];
            if (tok < 0 && run > t) tok = idx + k;
          }
          if (tok >= 0 && tok < V) sm.tok = tok;
        }
        done = true;
      } else {
        pre += tot;
      }
    }
  }
  __syncthreads();
  res.tok = sm.tok;
  __syncthreads();
  return res;
}

__device__ __forceinline__ float bits_f32(int b) {
  union { int i; float f; } v;
  v.i = b;
  return v.f;
}

// logits [n, V] + samp [5, n] (temperature bits, top_p bits, top_k,
// seed_lo, seed_hi) + counter [n] -> tokens int64 [n], tau fp32 [n].
template <int NT>
__global__ __launch_bounds__(NT) void sample_tokens_kernel(
    const unsigned short* __restrict__ logits, int V, long long n,
    const int* __restrict__ samp, const int* __restrict__ counter,
    long long* __restrict__ tokens, float* __restrict__ tau) {
  __shared__ SampleSmem<NT> sm;
  const long long i = blockIdx.x;
  const SampleResult r = sample_row<NT>(
      logits + i * V, V, bits_f32(samp[0 * n + i]), bits_f32(samp[1 * n + i]),
      samp[2 * n + i], (unsigned)samp[3 * n + i], (unsigned)samp[4 * n + i],
      (unsigned)counter[i], sm);
  if (threadIdx.x == 0) {
    tokens[i] = (long long)r.tok;
    tau[i] = r.tau;
  }
}

// Same sampling, then the state bump of decode_advance_kernel: ring
// store at ctr % chunk, stage[0] = tok, stage[1]/[3]/[4] += 1.  The
// Philox counter is stage[1] (the input token's position) before the
// bump.
template <int NT>
__global__ __launch_bounds__(NT) void decode_sample_advance_kernel(
    const unsigned short* __restrict__ logits, int V,
    int* __restrict__ stage,         // [6, b] int32
    long long b, long long* __restrict__ ring,  // [chunk, b] int64
    const long long* __restrict__ ctr,          // [1]
    int chunk, const int* __restrict__ samp) {  // [5, b] int32
  __shared__ SampleSmem<NT> sm;
  const long long i = blockIdx.x;
  const SampleResult r = sample_row<NT>(
      logits + i * V, V, bits_f32(samp[0 * b + i]), bits_f32(samp[1 * b + i]),
      samp[2 * b + i], (unsigned)samp[3 * b + i], (unsigned)samp[4 * b + i],
      (unsigned)stage[1 * b + i], sm);
  if (threadIdx.x == 0) {
    long long slot = *ctr % chunk;
    if (slot < 0) slot += chunk;
    ring[slot * b + i] = (long long)r.tok;
    stage[0 * b + i] = r.tok;  // next token fed back into the graph
    stage[1 * b + i] += 1;     // positions
    stage[3 * b + i] += 1;     // pos
    stage[4 * b + i] += 1;     // kv_lens
  }
}

// One block of SAMPLE_THREADS per row.  256 threads per row was measured
// too and lost every mode by 1.7-2.7x (docs/BENCHMARKS.md).
#define SAMPLE_THREADS 1024

extern "C" void sample_tokens_launch(const void* logits, int V, long long n,
                                     const void* samp, const void* counter,
                                     void* tokens, void* tau,
                                     hipStream_t stream) {
  hipLaunchKernelGGL(sample_tokens_kernel<SAMPLE_THREADS>, dim3((unsigned)n),
                     dim3(SAMPLE_THREADS), 0, stream,
                     (const unsigned short*)logits, V, n, (const int*)samp,
                     (const int*)counter, (long long*)tokens, (float*)tau);
}

extern "C" void decode_sample_advance_launch(const void* logits, int V,
                                             void* stage, long long b,
                                             void* ring, const void* ctr,
                                             int chunk, const void* samp,
                                             hipStream_t stream) {
  hipLaunchKernelGGL(decode_sample_advance_kernel<SAMPLE_THREADS>,
                     dim3((unsigned)b), dim3(SAMPLE_THREADS), 0, stream,
                     (const unsigned short*)logits, V, (int*)stage, b,
                     (long long*)ring, (const long long*)ctr, chunk,
                     (const int*)samp);
}

// ---- token log-probabilities (docs/KERNELS.md "Token log-probabilities") --
// log-softmax of one row at temperature 1 with no filter: the value of
// one chosen token and the first N tokens in the total order (value
// descending, index ascending), N <= LOGPROB_TOP.  The row is read with
// the sampler's row_pass; Z is the sampler's fixed-point sum with scale
// log2(e), so lse is a pure function of the row's values: the same
// logits give the same numbers in every batch row and on every rank.
//
//   1. max and NaN detect       degenerate rows answer NaN and stop;
//   2. Z_q                      fused with the count histogram of the
//                               key's high byte when N > 0;
//   3. low-byte histogram       inside the chosen high bin -> tkey, the
//                               key of the N-th largest value (0 when
//                               N >= V: everything is above it);
//   4. gather                   keys above tkey (fewer than N, any order,
//                               LDS counter), then ties at tkey in index
//                               order up to the remaining quota: per-wave
//                               tie counts, a serial scan of the wave
//                               totals, and each wave with a quota walks
//                               its own segment with lane prefix counts;
//   5. rank sort                the <= 20 distinct (key, idx) pairs.
//
// Loops are bounded by V, the 256 bins or LOGPROB_TOP.  Outputs are plain
// vector stores; the only atomics are integer LDS adds.
#define LOGPROB_TOP 20

template <int NT>
struct LogprobSmem {
  u64 wsum[NT / WAVE];
  float wmax[NT / WAVE];
  int wnan[NT / WAVE];
  unsigned wtie[NT / WAVE];
  unsigned hcnt[256 * HR];
  unsigned bcnt[256];
  unsigned sel_digit;
  unsigned sel_cnt;
  unsigned gcount;
  unsigned gkey[LOGPROB_TOP];
  int gidx[LOGPROB_TOP];
  double lse;
};

__device__ __forceinline__ float logprob_of(float l, double lse) {
  return (float)((double)l - lse);
}

// One row with the whole block.  chosen is the token whose value goes to
// *lp; n_top < 0 turns the row off (nothing read, nothing written),
// n_top > LOGPROB_TOP counts as LOGPROB_TOP.  top_lp / top_id point at the
// row's LOGPROB_TOP entries; all of them are written.
template <int NT>
__device__ __forceinline__ void logprob_row(
    const unsigned short* __restrict__ row, int V, long long chosen,
    int n_top, float* __restrict__ lp, float* __restrict__ top_lp,
    int* __restrict__ top_id, LogprobSmem<NT>& sm) {
  constexpr int NW = NT / WAVE;
  if (n_top < 0) return;  // uniform over the block
  const int N = n_top < LOGPROB_TOP ? n_top : LOGPROB_TOP;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int seg = (int)((((long long)V + NW - 1) / NW + 2047) / 2048 * 2048);
  const int iters = seg / 512;
  const int base = wid * seg + lane * 8;
  const bool vec_ok = ((unsigned long long)row & 15ull) == 0;
  const float qnan = __builtin_nanf("");

  // ---- 1. max and NaN detect -----------------------------------------
  float best = -INFINITY;
  int has_nan = 0;
  row_pass(row, V, vec_ok, base, iters,
           [&](int, unsigned short h, bool valid) {
             const float v = bf2f(h);
             if (valid && v > best) best = v;
             has_nan |= (valid && v != v);
           });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    best = fmaxf(best, __shfl_xor(best, off, WAVE));
    has_nan |= __shfl_xor(has_nan, off, WAVE);
  }
  if (lane == 0) {
    sm.wmax[wid] = best;
    sm.wnan[wid] = has_nan;
  }
  if (threadIdx.x == 0) sm.gcount = 0u;
  __syncthreads();
  best = sm.wmax[0];
  has_nan = sm.wnan[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    best = fmaxf(best, sm.wmax[w]);
    has_nan |= sm.wnan[w];
  }
  const float m = best;
  if (has_nan || !(fabsf(m) < INFINITY)) {
    if (threadIdx.x == 0) *lp = qnan;
    if (threadIdx.x < LOGPROB_TOP) {
      top_lp[threadIdx.x] = qnan;
      top_id[threadIdx.x] = -1;
    }
    return;
  }

  // ---- 2./3. Z_q and the threshold key -------------------------------
  // The sampler's radix walk with its top-k predicate "count at or above
  // this digit >= N", counts only.  N < V here, so the predicate holds at
  // digit 0 of either level and exactly one digit d has it while d + 1
  // does not.
  const float scale = 1.44269504088896340736f;
  const bool walk = N > 0 && N < V;
  const int copy = lane & (HR - 1);
  unsigned prefix = 0;
  unsigned cnt_above = 0;
  u64 zq = 0;
#pragma unroll 1
  for (int level = 0; level < (walk ? 2 : 1); ++level) {
    if (walk) {
      for (int i = threadIdx.x; i < 256 * HR; i += NT) sm.hcnt[i] = 0u;
      __syncthreads();
    }
    const int shift = level == 0 ? 8 : 0;
    row_pass(row, V, vec_ok, base, iters,
             [&](int, unsigned short h, bool valid) {
               if (level == 0)
                 zq += valid ? weight_q(bf2f(h), m, scale) : 0ull;
               const unsigned key = bf_key(h);
               if (walk && valid && (level == 0 || (key >> 8) == prefix))
                 atomicAdd(&sm.hcnt[((key >> shift) & 255u) * HR + copy], 1u);
             });
    if (level == 0) {
      zq = wave_sum_u64(zq);
      if (lane == 0) sm.wsum[wid] = zq;
    }
    __syncthreads();
    if (level == 0 && threadIdx.x == 0) {
      u64 z = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) z += sm.wsum[w];
      // z >= 2^40: the maximum's own weight
      sm.lse = (double)m + log((double)z * 9.094947017729282379150390625e-13);
    }
    if (!walk) break;
    if (threadIdx.x < 256) {
      unsigned c = 0;
#pragma unroll
      for (int r = 0; r < HR; ++r) c += sm.hcnt[threadIdx.x * HR + r];
      sm.bcnt[threadIdx.x] = c;
    }
    __syncthreads();
    if (threadIdx.x < 256) {
      const int d = threadIdx.x;
      unsigned c0 = cnt_above, c1 = cnt_above;  // at or above d / d + 1
      for (int e = 255; e >= 0; --e) {
        const unsigned c = sm.bcnt[e];
        if (e >= d) c0 += c;
        if (e > d) c1 += c;
      }
      if (c0 >= (unsigned)N && c1 < (unsigned)N) {
        sm.sel_digit = (unsigned)d;
        sm.sel_cnt = c1;
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | sm.sel_digit;
    cnt_above = sm.sel_cnt;
  }
  __syncthreads();
  const double lse = sm.lse;
  const unsigned tkey = walk ? prefix : 0u;

  // chosen token: bounds-checked, so an id outside [0, V) reads nothing
  if (threadIdx.x == 0)
    *lp = (chosen >= 0 && chosen < (long long)V)
              ? logprob_of(bf2f(row[chosen]), lse)
              : qnan;
  if (N == 0) {
    if (threadIdx.x < LOGPROB_TOP) {
      top_lp[threadIdx.x] = qnan;
      top_id[threadIdx.x] = -1;
    }
    return;
  }

  // ---- 4. gather --------------------------------------------------------
  // Above tkey: cnt_above < N elements (all V <= N of them when the walk
  // was skipped; every key of a NaN-free row is above 0).
  unsigned ties = 0;
  row_pass(row, V, vec_ok, base, iters,
           [&](int j, unsigned short h, bool valid) {
             const unsigned key = bf_key(h);
             if (valid && key > tkey) {
               const unsigned p = atomicAdd(&sm.gcount, 1u);
               if (p < LOGPROB_TOP) {
                 sm.gkey[p] = key;
                 sm.gidx[p] = j;
               }
             }
             ties += (walk && valid && key == tkey) ? 1u : 0u;
           });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ties += __shfl_xor(ties, off, WAVE);
  if (lane == 0) sm.wtie[wid] = ties;
  __syncthreads();
  const int total = walk ? N : V;  // entries reported: min(N, V)
  if (walk) {
    // Ties at tkey in index order: wave w's segment precedes wave w + 1's.
    const unsigned quota = (unsigned)N - cnt_above;  // >= 1
    unsigned before = 0;
    for (int w = 0; w < wid; ++w) before += sm.wtie[w];
    unsigned mine = 0;  // ties this wave admits
    if (before < quota) {
      mine = quota - before;
      if (mine > sm.wtie[wid]) mine = sm.wtie[wid];
    }
    unsigned run = 0;  // ties of this wave before the current step
    for (int it = 0; it < iters && run < mine; ++it) {
      const int idx = base + it * 512;
      const s16x8 x = load8(row, V, vec_ok, idx);
      unsigned c = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        c += (idx + k < V && bf_key((unsigned short)x[k]) == tkey) ? 1u : 0u;
      unsigned incl = c;
#pragma unroll
      for (int off = 1; off < WAVE; off <<= 1) {
        const unsigned o = __shfl_up(incl, off, WAVE);
        if (lane >= off) incl += o;
      }
      unsigned r = run + incl - c;  // rank of this lane's first tie
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (idx + k < V && bf_key((unsigned short)x[k]) == tkey) {
          if (r < mine) {
            const unsigned p = cnt_above + before + r;  // < N
            sm.gkey[p] = tkey;
            sm.gidx[p] = idx + k;
          }
          ++r;
        }
      }
      run += __shfl(incl, WAVE - 1, WAVE);
    }
  }
  __syncthreads();

  // ---- 5. rank sort and store -------------------------------------------
  if (threadIdx.x < LOGPROB_TOP) {
    const int t = threadIdx.x;
    if (t < total) {
      const unsigned key = sm.gkey[t];
      const int idx = sm.gidx[t];
      int rank = 0;
      for (int s = 0; s < total; ++s) {
        const unsigned ks = sm.gkey[s];
        rank += (ks > key || (ks == key && sm.gidx[s] < idx)) ? 1 : 0;
      }
      top_lp[rank] = logprob_of(key_value(key), lse);
      top_id[rank] = idx;
    } else {
      top_lp[t] = qnan;
      top_id[t] = -1;
    }
  }
}

// logits [n, V], ids int64 [n], n_top int32 [n] -> lp fp32 [n],
// top_lp fp32 [n, 20], top_ids int32 [n, 20].
template <int NT>
__global__ __launch_bounds__(NT) void token_logprobs_kernel(
    const unsigned short* __restrict__ logits, int V,
    const long long* __restrict__ ids, const int* __restrict__ n_top,
    float* __restrict__ lp, float* __restrict__ top_lp,
    int* __restrict__ top_ids) {
  __shared__ LogprobSmem<NT> sm;
  const long long i = blockIdx.x;
  logprob_row<NT>(logits + i * V, V, ids[i], n_top[i], lp + i,
                  top_lp + i * LOGPROB_TOP, top_ids + i * LOGPROB_TOP, sm);
}

// The in-graph form, launched after the advance kernel and before the
// ctr increment: the chosen token is stage[0], which the advance kernel
// has just written, and the ring row is the one it stored its token in.
// stage is only read.
template <int NT>
__global__ __launch_bounds__(NT) void decode_logprobs_kernel(
    const unsigned short* __restrict__ logits, int V,
    const int* __restrict__ stage, long long b,
    const int* __restrict__ n_top, float* __restrict__ lp_ring,
    float* __restrict__ top_lp_ring, int* __restrict__ top_id_ring,
    const long long* __restrict__ ctr, int chunk) {
  __shared__ LogprobSmem<NT> sm;
  const long long i = blockIdx.x;
  long long slot = *ctr % chunk;
  if (slot < 0) slot += chunk;
  const long long o = slot * b + i;
  logprob_row<NT>(logits + i * V, V, (long long)stage[i], n_top[i],
                  lp_ring + o, top_lp_ring + o * LOGPROB_TOP,
                  top_id_ring + o * LOGPROB_TOP, sm);
}

extern "C" void token_logprobs_launch(const void* logits, int V, long long n,
                                      const void* ids, const void* n_top,
                                      void* lp, void* top_lp, void* top_ids,
                                      hipStream_t stream) {
  hipLaunchKernelGGL(token_logprobs_kernel<SAMPLE_THREADS>, dim3((unsigned)n),
                     dim3(SAMPLE_THREADS), 0, stream,
                     (const unsigned short*)logits, V, (const long long*)ids,
                     (const int*)n_top, (float*)lp, (float*)top_lp,
                     (int*)top_ids);
}

extern "C" void decode_logprobs_launch(const void* logits, int V,
                                       const void* stage, long long b,
                                       const void* n_top, void* lp_ring,
                                       void* top_lp_ring, void* top_id_ring,
                                       const void* ctr, int chunk,
                                       hipStream_t stream) {
  hipLaunchKernelGGL(decode_logprobs_kernel<SAMPLE_THREADS>,
                     dim3((unsigned)b), dim3(SAMPLE_THREADS), 0, stream,
                     (const unsigned short*)logits, V, (const int*)stage, b,
                     (const int*)n_top, (float*)lp_ring, (float*)top_lp_ring,
                     (int*)top_id_ring, (const long long*)ctr, chunk);
}
