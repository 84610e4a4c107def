// Shared by the two NMS modes of Detect (detect.hip: fast NMS, detect_greedy.hip: traditional NMS), which must never drift apart:
// the order-preserving score keys and the box decode in the reference's exact op order.  Build with -ffp-contract=off.
#pragma once
#include "common.h"

__device__ __forceinline__ unsigned f2key(float f) {
  // order-preserving float -> uint (larger float => larger key); never 0 for finite inputs
  unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// decode(loc, prior) exactly as box_utils.py:304-310 evaluates it (left to right, fp32):
//   c = p.xy + (loc.xy * 0.1) * p.wh ; s = p.wh * exp(loc.wh * 0.2) ; xy1 = c - s/2 ; xy2 = s + xy1
__device__ __forceinline__ f32x4 decode_box(const float *loc, const float *pr) {
  const float cx = pr[0] + (loc[0] * 0.1f) * pr[2];
  const float cy = pr[1] + (loc[1] * 0.1f) * pr[3];
  const float w = pr[2] * expf(loc[2] * 0.2f);
  const float h = pr[3] * expf(loc[3] * 0.2f);
  f32x4 b;
  b[0] = cx - w / 2.f;
  b[1] = cy - h / 2.f;
  b[2] = w + b[0];
  b[3] = h + b[1];
  return b;
}
