// Shared by the MultiBoxLoss kernels (match.hip, mask_loss.hip, class_loss.hip, segm_loss.hip): their reductions, the per-image
// ranges, the workspace layout and the launch step.  The losses promise "the same inputs give the same bits", and a sum's bits are
// its ORDER OF ADDITIONS.  That order is this header's contract; nothing below may be re-associated:
//   a wave        the butterfly over lane distances 32, 16, 8, 4, 2, 1                               (ymi_wave_sum)
//   a block       its waves in wave order: w0 + w1 for 128 threads, ((w0 + w1) + w2) + w3 for 256    (ymi_waves_sum)
//                 integer counts: c0 + c1, (c0 + c1) + (c2 + c3)                                     (ymi_waves_count)
//   the loss      256 threads: thread t adds src[t], src[t + 256], .. in that order, then a tree over distances 128, 64, .. 1 in
//                 which slot t takes slot t + d                                                      (ymi_sum256)
//   chunk / tile partials: ascending index from +0.0                                                  (ymi_chunk_sum)
// What a term does to the total (alpha, alpha / mh / mw, a precomputed alpha / HW) stays in its own *_sum_k: those roundings differ.
#pragma once
#include "common.h"

__device__ __forceinline__ float ymi_qnan() { return __int_as_float(0x7fc00000); }

// the wave's sum in every lane
template <typename T> __device__ __forceinline__ T ymi_wave_sum(T v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// how many lanes of the wave hold `pred`, in every lane
__device__ __forceinline__ int ymi_wave_count(bool pred) { return __popcll(__ballot(pred)); }

// the per-wave values of a WAVES-wave block (lw[w], written by each wave's lane 0 before a barrier) in wave order
template <int WAVES> __device__ __forceinline__ float ymi_waves_sum(const float *lw) {
  static_assert(WAVES == 2 || WAVES == 4, "128- or 256-thread blocks");
  return WAVES == 2 ? lw[0] + lw[1] : ((lw[0] + lw[1]) + lw[2]) + lw[3];
}
template <int WAVES> __device__ __forceinline__ int ymi_waves_count(const int *cw) {
  static_assert(WAVES == 2 || WAVES == 4, "128- or 256-thread blocks");
  return WAVES == 2 ? cw[0] + cw[1] : (cw[0] + cw[1]) + (cw[2] + cw[3]);
}

// the sum of l over a WAVES-wave block, for thread 0 to use (lw: WAVES floats of LDS; one barrier, reached by every thread)
template <int WAVES> __device__ __forceinline__ float ymi_block_sum(float l, float *lw) {
  l = ymi_wave_sum(l);
  if ((threadIdx.x & 63) == 0) lw[threadIdx.x >> 6] = l;
  __syncthreads();
  return ymi_waves_sum<WAVES>(lw);
}

// one block of 256 threads: the sum of src[0 .. total), in every thread
__device__ __forceinline__ float ymi_sum256(const float *src, long total) {
  __shared__ float part[256];
  const int t = threadIdx.x;
  float s = 0.f;
  for (long k = t; k < total; k += 256) s += src[k];
  part[t] = s;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (t < d) part[t] += part[t + d];
    __syncthreads();
  }
  return part[0];
}

// element i of the n partials ws[c * stride + i] that an earlier launch left in the workspace, one per chunk or tile c
__device__ __forceinline__ float ymi_chunk_sum(const float *ws, size_t stride, int n, size_t i) {
  float s = 0.f;
  for (int c = 0; c < n; ++c) s += ws[c * stride + i];
  return s;
}

// image b's rows [g0, g0 + n) from device offsets nobody validated on the device: never outside [0, total), never more than cap
__device__ __forceinline__ void ymi_image_range(const int32_t *off, int b, int total, int &g0, int &n, int cap = 0x7fffffff) {
  int a = off[b], e = off[b + 1];
  a = a < 0 ? 0 : (a > total ? total : a);
  e = e < a ? a : (e > total ? total : e);
  g0 = a; n = e - a > cap ? cap : e - a;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// bytes of a workspace part of n 4-byte elements: parts start 16 bytes aligned
static inline int64_t ymi_ws_part(int64_t n) { return (4 * n + 15) / 16 * 16; }

// element counts of the parts in, their byte offsets out; returns the total
template <int K> static inline int64_t ymi_ws_layout(const int64_t (&sizes)[K], int64_t (&off)[K]) {
  int64_t at = 0;
  for (int k = 0; k < K; ++k) { off[k] = at; at += ymi_ws_part(sizes[k]); }
  return at;
}

// [off[b], off[b+1]) covers [0, total) image by image; each image holds lo..hi rows
static inline int ymi_validate_offsets(const int32_t *off, int B, int total, int lo, int hi) {
  if (off[0] != 0 || off[B] != total) return YMI_EARG;
  for (int b = 0; b < B; ++b) {
    const long n = (long)off[b + 1] - off[b];
    if (n < lo || n > hi) return YMI_EARG;
  }
  return YMI_OK;
}

// one launch and its status; an entry point chains them: rc = ymi_launch(..); if (!rc) rc = ymi_launch(..); .. return rc;
template <typename P> static inline int ymi_launch(void (*kernel)(P), dim3 grid, dim3 block, size_t lds, void *stream, const P &p) {
  hipLaunchKernelGGL(kernel, grid, block, lds, (hipStream_t)stream, p);
  return ymi_launch_status();
}
