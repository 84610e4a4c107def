// BatchNorm2d on its own, forward and backward, NHWC fp32 viewed as [npos, C] (C % 4 == 0), for the train-mode backbone
// (backbone.py:37-57; the inference plan folds BatchNorm into the filters and never computes it).  No atomics: the same inputs give the
// same bits.
//
//   ymi_bn_fwd_nhwc_f32   training = 1: the batch statistics over npos, y = gamma (x - mean) invstd + beta (+ res) (ReLU), mean and invstd
//                         saved, the running statistics updated as PyTorch does; training = 0: the same map with the running statistics.
//   ymi_bn_bwd_nhwc_f32   gh = dy [y > 0], d_res = gh, dbeta = sum gh, dgamma = sum gh xh (xh = (x - mean) invstd),
//                         dx = gamma invstd (gh - dbeta / npos - xh dgamma / npos) (training) or gamma invstd gh (frozen).
//
// THE COLUMN SUMS (the order is the contract): the positions are cut into nchunks chunks of `per` positions (bn_plan: a function of
// npos only).  A thread owns (chunk, 4 channels) and adds its chunk's positions in ascending order from +0.0; the chunk partials go to
// the workspace, and a second launch adds them per channel with one wave per channel: lane l adds the chunks l, l + 64, .. in ascending
// order from +0.0, then the 64 lane sums are added by the butterfly over the lane distances 32, 16, 8, 4, 2, 1 (loss_common.h
// ymi_wave_sum).
//
// THE VARIANCE comes from deviations about the mean, never from E[x^2] - E[x]^2.  The first pass sums x - pivot with pivot = x[0, c]
// (for data that sits far from 0 with a small spread these differences are exact and small, so the sum loses nothing) and yields
// delta = sum / npos, mean = pivot + delta; the second pass sums ((x - pivot) - delta)^2.  The normalisation uses the same two-part
// deviation (x - pivot) - delta, which does not see the rounding of mean to fp32; the saved mean is the rounded sum.
//
//   ymi_bn_leaky_fwd_nhwc_f32 / ymi_bn_leaky_bwd_nhwc_f32   the same pair for the DarkNet unit (BatchNorm2d, LeakyReLU(0.1)) and the
//                         DarkNetBlock's `conv2(conv1(x)) + x`: z = gamma (x - mean) invstd + beta, a = z > 0 ? z : 0.1f * z (one fp32
//                         multiply), y = a + res: the residual comes AFTER the activation.  Backward: gh = z > 0 ? dy : 0.1f * dy, then
//                         dbeta, dgamma and dx by the formulas, chunks and order of additions above; d_res is dy itself and no kernel
//                         writes it.  The statistics, mean / invstd, the running update and the column sums are the kernels above.
//
// THE SLOPE DECISION is made once, by the forward.  Without a residual y > 0 is exactly z > 0 (0.1f * z is never positive for z <= 0 and
// y = z for z > 0), so the backward reads it from y.  With a residual it cannot be read from y, and the forward writes it down: bit
// (i & 31) of word i >> 5 of `mask` is z > 0 of element i of the [npos, C] map, ceil(npos C / 32) words, 1/32 of the map.  A thread owns
// four consecutive elements, so eight neighbouring lanes OR their nibbles together over the lane distances 1, 2, 4 and the first of the
// eight stores the word: every word is written exactly once, the bits past the last element are 0.  The backward reads the bit and
// never recomputes z, so no rounding can flip a decision between the two directions.
//
// Launches: forward, training: bn_sum_k, bn_delta_k, bn_var_k, bn_fin_k, bn_apply_k; frozen: bn_fin_k, bn_apply_k.  Backward:
// bn_bwd_sum_k, bn_bwd_fin_k (both skipped when frozen and neither dgamma nor dbeta is asked for), bn_bwd_apply_k (skipped when
// neither dx nor d_res is asked for).
#include <initializer_list>
#include "loss_common.h"
#include "../../include/yolact_amd.h"

namespace {

struct BnParams {
  const float *x, *res, *gamma, *beta, *dy, *yin;
  float *y, *mean, *invstd, *rmean, *rvar, *dx, *dres, *dgamma, *dbeta;
  float *part0, *part1, *fin0, *fin1;                  // [nchunks][C] twice, [C] twice (forward: pivot, delta; backward: dbeta, dgamma)
  uint32_t *mask;                                      // leaky forward: the decisions z > 0, or NULL
  const uint32_t *maskin;                              // leaky backward: the same words, or NULL (then y is read)
  long npos, per;
  int C, C4, nchunks, training, relu;
  float eps, momentum;
};

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, const f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// thread = (chunk, 4 channels): sum of x - pivot over the chunk's positions
__global__ __launch_bounds__(256) void bn_sum_k(const BnParams p) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  const int chunk = (int)(id / p.C4), c = 4 * (int)(id - (long)chunk * p.C4);
  if (chunk >= p.nchunks) return;
  const long r0 = chunk * p.per, r1 = r0 + p.per < p.npos ? r0 + p.per : p.npos;
  const f32x4 piv = ld4(p.x + c);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (long r = r0; r < r1; ++r) s += ld4(p.x + (size_t)r * p.C + c) - piv;
  st4(p.part0 + (size_t)chunk * p.C + c, s);
}

// The chunk partials of channel c, in every lane of the wave that owns the channel: lane l adds the chunks l, l + 64, .. in ascending
// order from +0.0, then the butterfly of loss_common.h adds the 64 lane sums (a column of 1024 partials is 16 dependent loads, not 1024)
__device__ __forceinline__ float bn_col_sum(const float *part, int nchunks, int C, int c) {
  float s = 0.f;
  for (int k = (int)(threadIdx.x & 63); k < nchunks; k += 64) s += part[(size_t)k * C + c];
  return ymi_wave_sum(s);
}

// wave = channel (4 per block): pivot and delta = (the chunk sums) / npos
__global__ __launch_bounds__(256) void bn_delta_k(const BnParams p) {
  const int c = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (c >= p.C) return;                                // (wave-uniform)
  const float s = bn_col_sum(p.part0, p.nchunks, p.C, c);
  if ((threadIdx.x & 63) != 0) return;
  p.fin0[c] = p.x[c];
  p.fin1[c] = s / (float)p.npos;
}

// thread = (chunk, 4 channels): sum of ((x - pivot) - delta)^2
__global__ __launch_bounds__(256) void bn_var_k(const BnParams p) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  const int chunk = (int)(id / p.C4), c = 4 * (int)(id - (long)chunk * p.C4);
  if (chunk >= p.nchunks) return;
  const long r0 = chunk * p.per, r1 = r0 + p.per < p.npos ? r0 + p.per : p.npos;
  const f32x4 piv = ld4(p.fin0 + c), del = ld4(p.fin1 + c);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (long r = r0; r < r1; ++r) {
    const f32x4 d = (ld4(p.x + (size_t)r * p.C + c) - piv) - del;
    s += d * d;
  }
  st4(p.part1 + (size_t)chunk * p.C + c, s);
}

// wave = channel (4 per block): mean, invstd, the running statistics (training); the running statistics as mean / invstd (frozen)
__global__ __launch_bounds__(256) void bn_fin_k(const BnParams p) {
  const int c = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (c >= p.C) return;                                // (wave-uniform)
  const bool first = (threadIdx.x & 63) == 0;
  if (!p.training) {
    if (!first) return;
    const float m = p.rmean[c];
    p.fin0[c] = m;
    p.fin1[c] = 0.f;
    p.mean[c] = m;
    p.invstd[c] = 1.f / sqrtf(p.rvar[c] + p.eps);
    return;
  }
  const float s = bn_col_sum(p.part1, p.nchunks, p.C, c);
  if (!first) return;
  const float n = (float)p.npos;
  const float var = s / n, m = p.fin0[c] + p.fin1[c];
  p.mean[c] = m;
  p.invstd[c] = 1.f / sqrtf(var + p.eps);
  if (p.rmean) p.rmean[c] = (1.f - p.momentum) * p.rmean[c] + p.momentum * m;
  if (p.rvar) p.rvar[c] = (1.f - p.momentum) * p.rvar[c] + p.momentum * (s / (n - 1.f));
}

constexpr float BN_SLOPE = 0.1f;                      // nn.LeakyReLU(0.1)

// thread = (position, 4 channels).  LEAKY: LeakyReLU(0.1) and then the residual, in place of the residual and then ReLU; the
// decisions z > 0 go to p.mask when there is one
template <bool LEAKY> __global__ __launch_bounds__(256) void bn_apply_k(const BnParams p) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = id < p.npos * p.C4;
  if (!LEAKY && !live) return;
  unsigned bits = 0u;
  if (live) {
    const int c = 4 * (int)(id % p.C4);
    const size_t o = (size_t)id * 4;
    const f32x4 d = (ld4(p.x + o) - ld4(p.fin0 + c)) - ld4(p.fin1 + c);
    f32x4 v = d * ld4(p.invstd + c) * ld4(p.gamma + c) + ld4(p.beta + c);
    if (LEAKY) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool pos = v[e] > 0.f;
        bits |= (pos ? 1u : 0u) << e;
        v[e] = pos ? v[e] : BN_SLOPE * v[e];
      }
      if (p.res) v += ld4(p.res + o);
    } else {
      if (p.res) v += ld4(p.res + o);
      if (p.relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
      }
    }
    st4(p.y + o, v);
  }
  if (LEAKY && p.mask) {                               // (uniform: every lane of the wave, live or not, takes part in the exchange)
    bits <<= 4 * (threadIdx.x & 7);
#pragma unroll
    for (int dl = 1; dl <= 4; dl <<= 1) bits |= (unsigned)__shfl_xor((int)bits, dl);
    if (live && (threadIdx.x & 7) == 0) p.mask[id >> 3] = bits;      // the first of eight lanes is live whenever one of them is
  }
}

// gh of four consecutive elements.  LEAKY: the forward's decision from its mask, or from y where there was no residual
template <bool LEAKY> __device__ __forceinline__ f32x4 bn_gh(const BnParams &p, size_t o) {
  f32x4 g = ld4(p.dy + o);
  if (LEAKY) {
    if (p.maskin) {
      const unsigned bits = p.maskin[o >> 5] >> (o & 31);
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = (bits >> e & 1u) ? g[e] : BN_SLOPE * g[e];
    } else {
      const f32x4 y = ld4(p.yin + o);
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = y[e] > 0.f ? g[e] : BN_SLOPE * g[e];
    }
  } else if (p.relu) {
    const f32x4 y = ld4(p.yin + o);
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = y[e] > 0.f ? g[e] : 0.f;
  }
  return g;
}

// thread = (chunk, 4 channels): sums of gh and of gh xh
template <bool LEAKY> __global__ __launch_bounds__(256) void bn_bwd_sum_k(const BnParams p) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  const int chunk = (int)(id / p.C4), c = 4 * (int)(id - (long)chunk * p.C4);
  if (chunk >= p.nchunks) return;
  const long r0 = chunk * p.per, r1 = r0 + p.per < p.npos ? r0 + p.per : p.npos;
  const f32x4 m = ld4(p.mean + c), is = ld4(p.invstd + c);
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
  for (long r = r0; r < r1; ++r) {
    const size_t o = (size_t)r * p.C + c;
    const f32x4 g = bn_gh<LEAKY>(p, o);
    s0 += g;
    s1 += g * ((ld4(p.x + o) - m) * is);
  }
  st4(p.part0 + (size_t)chunk * p.C + c, s0);
  st4(p.part1 + (size_t)chunk * p.C + c, s1);
}

// wave = channel (4 per block): the chunk partials (bn_col_sum)
__global__ __launch_bounds__(256) void bn_bwd_fin_k(const BnParams p) {
  const int c = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (c >= p.C) return;                                // (wave-uniform)
  const float s0 = bn_col_sum(p.part0, p.nchunks, p.C, c), s1 = bn_col_sum(p.part1, p.nchunks, p.C, c);
  if ((threadIdx.x & 63) != 0) return;
  p.fin0[c] = s0;
  p.fin1[c] = s1;
  if (p.dbeta) p.dbeta[c] = s0;
  if (p.dgamma) p.dgamma[c] = s1;
}

// thread = (position, 4 channels)
template <bool LEAKY> __global__ __launch_bounds__(256) void bn_bwd_apply_k(const BnParams p) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= p.npos * p.C4) return;
  const int c = 4 * (int)(id % p.C4);
  const size_t o = (size_t)id * 4;
  const f32x4 g = bn_gh<LEAKY>(p, o);
  if (p.dres) st4(p.dres + o, g);
  if (!p.dx) return;
  const f32x4 is = ld4(p.invstd + c), k = ld4(p.gamma + c) * is;
  if (p.training) {
    const float n = (float)p.npos;
    const f32x4 xh = (ld4(p.x + o) - ld4(p.mean + c)) * is;
    st4(p.dx + o, k * ((g - ld4(p.fin0 + c) / n) - xh * (ld4(p.fin1 + c) / n)));
  } else {
    st4(p.dx + o, k * g);
  }
}

struct BnPlan { long per; int nchunks; };

// chunks of at least 32 positions, at most 1024 of them: a function of npos only
BnPlan bn_plan(long npos) {
  BnPlan b;
  b.per = (npos + 1023) / 1024;
  if (b.per < 32) b.per = 32;
  b.nchunks = (int)((npos + b.per - 1) / b.per);
  return b;
}

int validate_bn(const ymi_bn_desc *d) {
  if (!d) return YMI_ENULL;
  if (d->npos < 1 || d->C < 1 || (d->training != 0 && d->training != 1) || (d->relu != 0 && d->relu != 1)) return YMI_EARG;
  if (d->training && d->npos < 2) return YMI_EARG;
  if (!(d->eps >= 0.f)) return YMI_EARG;
  if (d->C % 4 != 0 || d->npos >= (1L << 40) / d->C) return YMI_ESHAPE;
  return YMI_OK;
}

bool bn_misaligned(std::initializer_list<const void *> ps) {
  uintptr_t a = 0;
  for (const void *q : ps) a |= (uintptr_t)q;
  return (a & 15) != 0;
}

void bn_fill(BnParams &p, const ymi_bn_desc *d, const BnPlan &b) {
  p.x = d->x; p.res = d->res; p.gamma = d->gamma; p.beta = d->beta; p.dy = d->dy; p.yin = d->y;
  p.y = d->y; p.mean = d->mean; p.invstd = d->invstd; p.rmean = d->running_mean; p.rvar = d->running_var;
  p.dx = d->dx; p.dres = d->d_res; p.dgamma = d->dgamma; p.dbeta = d->dbeta;
  char *ws = static_cast<char *>(d->ws);
  const int64_t a = ymi_ws_part((int64_t)b.nchunks * d->C), c = ymi_ws_part(d->C);
  p.part0 = reinterpret_cast<float *>(ws); p.part1 = reinterpret_cast<float *>(ws + a);
  p.fin0 = reinterpret_cast<float *>(ws + 2 * a); p.fin1 = reinterpret_cast<float *>(ws + 2 * a + c);
  p.npos = d->npos; p.per = b.per; p.C = d->C; p.C4 = d->C / 4; p.nchunks = b.nchunks; p.training = d->training; p.relu = d->relu;
  p.eps = d->eps; p.momentum = d->momentum;
  p.mask = nullptr; p.maskin = nullptr;
}

}  // namespace

// Workspace of both entries: [nchunks][C] floats twice, then [C] floats twice
extern "C" int64_t ymi_bn_ws_bytes(const ymi_bn_desc *d) {
  const int rc = validate_bn(d);
  if (rc) return rc;
  const BnPlan b = bn_plan(d->npos);
  return 2 * ymi_ws_part((int64_t)b.nchunks * d->C) + 2 * ymi_ws_part(d->C);
}

namespace {

template <bool LEAKY> int bn_forward(const ymi_bn_desc *d, uint32_t *mask, void *stream) {
  const int rc = validate_bn(d);
  if (rc) return rc;
  if (LEAKY && d->relu) return YMI_EARG;
  if (!d->x || !d->gamma || !d->beta || !d->y || !d->mean || !d->invstd || !d->ws) return YMI_ENULL;
  if (!d->training && (!d->running_mean || !d->running_var)) return YMI_ENULL;
  if (LEAKY && d->res && !mask) return YMI_ENULL;
  if (bn_misaligned({d->x, d->res, d->gamma, d->beta, d->y, d->mean, d->invstd, d->ws, mask})) return YMI_ESHAPE;
  if (d->ws_bytes < ymi_bn_ws_bytes(d)) return YMI_ESHAPE;
  const BnPlan b = bn_plan(d->npos);
  BnParams p;
  bn_fill(p, d, b);
  p.mask = mask;
  const dim3 blk(256);
  const dim3 gchunk((unsigned)(((long)b.nchunks * p.C4 + 255) / 256)), gcol((unsigned)((d->C + 3) / 4));
  const dim3 gall((unsigned)((d->npos * p.C4 + 255) / 256));
  int rl = YMI_OK;
  if (d->training) {
    rl = ymi_launch(bn_sum_k, gchunk, blk, 0, stream, p);
    if (!rl) rl = ymi_launch(bn_delta_k, gcol, blk, 0, stream, p);
    if (!rl) rl = ymi_launch(bn_var_k, gchunk, blk, 0, stream, p);
  }
  if (!rl) rl = ymi_launch(bn_fin_k, gcol, blk, 0, stream, p);
  if (!rl) rl = ymi_launch(bn_apply_k<LEAKY>, gall, blk, 0, stream, p);
  return rl;
}

template <bool LEAKY> int bn_backward(const ymi_bn_desc *d, const uint32_t *mask, void *stream) {
  const int rc = validate_bn(d);
  if (rc) return rc;
  if (LEAKY && (d->relu || d->d_res)) return YMI_EARG;
  const bool sums = d->training || d->dgamma || d->dbeta, apply = d->dx || d->d_res;
  if (!sums && !apply) return YMI_ENULL;
  if (!d->dy || (d->relu && !d->y) || (LEAKY && !mask && !d->y) || !d->ws) return YMI_ENULL;
  if ((sums || d->dx) && (!d->x || !d->mean || !d->invstd)) return YMI_ENULL;
  if (d->dx && !d->gamma) return YMI_ENULL;
  if (bn_misaligned({d->x, d->dy, d->y, d->gamma, d->mean, d->invstd, d->dx, d->d_res, d->dgamma, d->dbeta, d->ws, mask})) return YMI_ESHAPE;
  if (d->ws_bytes < ymi_bn_ws_bytes(d)) return YMI_ESHAPE;
  const BnPlan b = bn_plan(d->npos);
  BnParams p;
  bn_fill(p, d, b);
  p.maskin = mask;
  const dim3 blk(256);
  int rl = YMI_OK;
  if (sums) {
    rl = ymi_launch(bn_bwd_sum_k<LEAKY>, dim3((unsigned)(((long)b.nchunks * p.C4 + 255) / 256)), blk, 0, stream, p);
    if (!rl) rl = ymi_launch(bn_bwd_fin_k, dim3((unsigned)((d->C + 3) / 4)), blk, 0, stream, p);
  }
  if (!rl && apply) rl = ymi_launch(bn_bwd_apply_k<LEAKY>, dim3((unsigned)((d->npos * p.C4 + 255) / 256)), blk, 0, stream, p);
  return rl;
}

}  // namespace

extern "C" int ymi_bn_fwd_nhwc_f32(const ymi_bn_desc *d, void *stream) { return bn_forward<false>(d, nullptr, stream); }
extern "C" int ymi_bn_bwd_nhwc_f32(const ymi_bn_desc *d, void *stream) { return bn_backward<false>(d, nullptr, stream); }

// LeakyReLU(0.1) with the residual behind it (the header comment); `mask`: ceil(npos C / 32) words, needed with a residual
extern "C" int ymi_bn_leaky_fwd_nhwc_f32(const ymi_bn_desc *d, uint32_t *mask, void *stream) { return bn_forward<true>(d, mask, stream); }
extern "C" int ymi_bn_leaky_bwd_nhwc_f32(const ymi_bn_desc *d, const uint32_t *mask, void *stream) {
  return bn_backward<true>(d, mask, stream);
}
