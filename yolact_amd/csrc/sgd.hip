// The SGD update of a whole parameter group in one launch (train.py:215-216,316-318: optimizer.step() behind the isfinite(loss) test,
// and optimizer.zero_grad()).  The contract (formulas, op order, guard, error codes) is the comment of ymi_sgd_step_f32 in
// include/yolact_amd.h.
//
// A multi-tensor apply: the device holds a table of tensors {p, g, m, n} and a table of chunks {tensor, first}; block b walks the chunks
// b, b + grid, ... (grid <= 2048: the kernel is memory bound, 3 reads and 2-3 writes per element, nothing is reused), 256 threads, a
// chunk of YMI_SGD_CHUNK = 4096 elements = four 16-byte lanes per thread: all twelve loads of a full chunk are issued before the first
// result is needed.  A chunk starts a multiple of 4096 elements into its tensor, so it is 16-byte aligned exactly when the tensor is;
// a tensor that is not (a view one element into a buffer) goes one element at a time.  Every operation is __fmul_rn / __fadd_rn /
// __fsub_rn: rounded once, never contracted.  The guard's scalar is one uniform load per block.  No atomics, no LDS.
#include "common.h"
#include "../../include/yolact_amd.h"
#include <cmath>

namespace {

constexpr int SGD_THREADS = 256;
constexpr int SGD_LANES = YMI_SGD_CHUNK / 4 / SGD_THREADS;      // 16-byte lanes per thread and chunk
constexpr int SGD_DEFAULT_BLOCKS = 2048;
static_assert(YMI_SGD_CHUNK % 4 == 0 && SGD_LANES * 4 * SGD_THREADS == YMI_SGD_CHUNK, "a chunk is whole 16-byte lanes per thread");

struct SgdParams {
  const ymi_sgd_tensor *tensors;
  const ymi_sgd_chunk *chunks;
  const float *loss;
  int32_t *skipped;
  int n_tensors, n_chunks;
  float lr, mom, wd;
};

template <bool MOM>
__device__ __forceinline__ void sgd_elem(float &p, float g, float &m, float lr, float mom, float wd) {
  float d = wd == 0.f ? g : __fadd_rn(g, __fmul_rn(wd, p));
  if (MOM) {
    m = __fadd_rn(__fmul_rn(mom, m), d);
    d = m;
  }
  p = __fsub_rn(p, __fmul_rn(lr, d));
}

template <bool MOM, bool ZERO>
__global__ __launch_bounds__(SGD_THREADS) void sgd_step_k(SgdParams q) {
  const int tid = threadIdx.x;
  bool apply = true;
  if (q.loss) {
    const float l = *q.loss;
    apply = fabsf(l) <= 3.402823466e+38f;      // false for inf and for NaN
  }
  if (!apply && q.skipped && blockIdx.x == 0 && tid == 0) *q.skipped = *q.skipped + 1;
  if (!apply && !ZERO) return;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int c = blockIdx.x; c < q.n_chunks; c += gridDim.x) {
    const ymi_sgd_chunk ch = q.chunks[c];
    if ((unsigned)ch.tensor >= (unsigned)q.n_tensors) continue;
    const ymi_sgd_tensor t = q.tensors[ch.tensor];
    if (ch.first < 0 || ch.first >= t.n || !t.p || !t.g || (MOM && !t.m)) continue;
    const int64_t left = t.n - ch.first;
    const int len = left < YMI_SGD_CHUNK ? (int)left : YMI_SGD_CHUNK;
    float *p = t.p + ch.first, *g = t.g + ch.first, *m = MOM ? t.m + ch.first : nullptr;
    const bool aligned = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0;
    if (!apply) {                              // a skipped step: only the gradients are written
      if (aligned) {
        const int n4 = len >> 2;
        for (int i = tid; i < n4; i += SGD_THREADS) reinterpret_cast<f32x4 *>(g)[i] = zero4;
        if (n4 * 4 + tid < len) g[n4 * 4 + tid] = 0.f;
      } else {
        for (int i = tid; i < len; i += SGD_THREADS) g[i] = 0.f;
      }
      continue;
    }
    if (aligned) {
      const int n4 = len >> 2;
      f32x4 *p4 = reinterpret_cast<f32x4 *>(p), *g4 = reinterpret_cast<f32x4 *>(g), *m4 = reinterpret_cast<f32x4 *>(m);
      f32x4 pv[SGD_LANES], gv[SGD_LANES], mv[SGD_LANES];
#pragma unroll
      for (int k = 0; k < SGD_LANES; ++k) {
        const int i = tid + k * SGD_THREADS;
        if (i < n4) {
          pv[k] = p4[i];
          gv[k] = g4[i];
          if (MOM) mv[k] = m4[i];
        }
      }
#pragma unroll
      for (int k = 0; k < SGD_LANES; ++k) {
        const int i = tid + k * SGD_THREADS;
        if (i < n4) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float pe = pv[k][j], me = MOM ? mv[k][j] : 0.f;
            sgd_elem<MOM>(pe, gv[k][j], me, q.lr, q.mom, q.wd);
            pv[k][j] = pe;
            if (MOM) mv[k][j] = me;
          }
          p4[i] = pv[k];
          if (MOM) m4[i] = mv[k];
          if (ZERO) g4[i] = zero4;
        }
      }
      const int i = n4 * 4 + tid;              // the tail: at most 3 elements
      if (i < len) {
        float pe = p[i], me = MOM ? m[i] : 0.f;
        sgd_elem<MOM>(pe, g[i], me, q.lr, q.mom, q.wd);
        p[i] = pe;
        if (MOM) m[i] = me;
        if (ZERO) g[i] = 0.f;
      }
    } else {
      for (int i = tid; i < len; i += SGD_THREADS) {
        float pe = p[i], me = MOM ? m[i] : 0.f;
        sgd_elem<MOM>(pe, g[i], me, q.lr, q.mom, q.wd);
        p[i] = pe;
        if (MOM) m[i] = me;
        if (ZERO) g[i] = 0.f;
      }
    }
  }
}

}  // namespace

extern "C" int64_t ymi_sgd_plan(const int64_t *numel, int n, ymi_sgd_chunk *out, int64_t cap) {
  if (n < 0 || (n > 0 && !numel) || cap < 0) return YMI_EARG;
  int64_t count = 0;
  for (int t = 0; t < n; ++t) {
    if (numel[t] < 0) return YMI_EARG;
    for (int64_t first = 0; first < numel[t]; first += YMI_SGD_CHUNK, ++count) {
      if (out && count < cap) out[count] = ymi_sgd_chunk{t, 0, first};
    }
  }
  return count;
}

extern "C" int ymi_sgd_step_f32(const ymi_sgd_desc *d, void *stream) {
  if (!d) return YMI_ENULL;
  if (!d->tensors || !d->chunks) return YMI_EARG;
  if (d->n_tensors < 0 || d->n_chunks < 0 || d->max_blocks < 0) return YMI_EARG;
  if (!(d->momentum >= 0.f) || !std::isfinite(d->momentum)) return YMI_EARG;
  if (d->tensors_host) {
    for (int t = 0; t < d->n_tensors; ++t) {
      const ymi_sgd_tensor &q = d->tensors_host[t];
      if (!q.p || !q.g || q.n < 0 || (d->momentum > 0.f && !q.m)) return YMI_EARG;
    }
  }
  const int cap = d->max_blocks > 0 ? d->max_blocks : SGD_DEFAULT_BLOCKS;
  const int grid = d->n_chunks < 1 ? 1 : (d->n_chunks < cap ? d->n_chunks : cap);      // one block still counts a skipped step
  SgdParams q{d->tensors, d->chunks, d->loss, d->skipped, d->n_tensors, d->n_chunks, d->lr, d->momentum, d->weight_decay};
  const bool mom = d->momentum > 0.f, zero = d->zero_grad != 0;
  const hipStream_t s = (hipStream_t)stream;
  if (mom && zero) hipLaunchKernelGGL((sgd_step_k<true, true>), dim3(grid), dim3(SGD_THREADS), 0, s, q);
  else if (mom) hipLaunchKernelGGL((sgd_step_k<true, false>), dim3(grid), dim3(SGD_THREADS), 0, s, q);
  else if (zero) hipLaunchKernelGGL((sgd_step_k<false, true>), dim3(grid), dim3(SGD_THREADS), 0, s, q);
  else hipLaunchKernelGGL((sgd_step_k<false, false>), dim3(grid), dim3(SGD_THREADS), 0, s, q);
  return ymi_launch_status();
}
