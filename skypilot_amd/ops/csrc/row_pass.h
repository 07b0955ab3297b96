// Row traversal of the one-workgroup-per-row decode kernels
// (decode_sample.hip, decode_penalty.hip): 16-byte loads of a bf16 row,
// four in flight per lane, with a bounds-checked scalar path for rows
// that do not start on a 16-byte boundary (odd V) and for the row tail,
// so that nothing at or past V is touched.
#pragma once

#include "common.h"

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

// The store that mirrors load8: positions >= V are not written.
__device__ __forceinline__ void store8(unsigned short* __restrict__ row, int V,
                                       bool vec_ok, int idx, s16x8 v) {
  if (vec_ok && idx + 8 <= V) {
    *(s16x8*)(row + idx) = v;
  } else if (idx < V) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (idx + k < V) row[idx + k] = (unsigned short)v[k];
  }
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
