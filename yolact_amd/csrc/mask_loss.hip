// The lincomb mask loss 'M' of MultiBoxLoss with both gradients in one pass (layers/modules/multibox_loss.py:499-627,650 for the
// switches both shipped base configs train with: crop, emulate-ROI-pooling normalisation, binarised GT, sigmoid; box_utils.py:328-373).
//
//     x = sum_k proto[b,r,c,k] * coef[j,k]     p = sigmoid(x)     q = inside_j(r,c) ? p : 0     l = BCE(q, t)
//     L_j = sum_{r,c} l  (roi_norm: / box width in pixels / box height in pixels * (crop ? mh*mw : 1))
//     loss = alpha / mh / mw * sum_j weight_j * L_j                  dl/dx = inside ? p - t : 0
//
// mask_loss_k is lincomb_common.h's ymi_lincomb_bwd with the term below: next to an instance's coefficients and window it stages
// d loss / d L_j and the clamped GT row (up to CAP_MAX = 320 instances at once), a wave also reduces its 64 values of l per instance,
// and the tile's partial of L_j goes to the workspace with that of d_coef.  Outside the window g = 0 and l = 100 t.
// mask_loss_dcoef_k sums the tile partials in tile order (d_coef, L_j); mask_loss_sum_k sums weight_j * L_j in a fixed tree.
//
// Numerics.  With lincomb_common.h's e = exp(-|x|) the inside-window BCE is softplus(-+x) = max(-+x, 0) + log1p(e), capped at the
// reference's 100.  For |x| <= 12 this is the reference's
// -max(log q, -100) to fp32 round-off (and closer to the exact value than log(1 - p) of a rounded p).  Beyond |x| ~ 17 the
// reference's fp32 sigmoid saturates to exactly 0 or 1, its BCE jumps to the clamp 100 and its gradient to 0; this kernel stays on
// the smooth branch there: l = min(softplus, 100), g = p - t.  Everything stays finite for any finite input.
#include "lincomb_common.h"
#include "../../include/yolact_amd.h"

namespace {

constexpr int JC = YMI_LINCOMB_JC;
constexpr int CAP_MAX = 320;    // instances staged in LDS at once (one reference config trains 300 per image)

struct MlParams {
  const float *proto, *coef, *box, *weight;
  const uint8_t *gt;
  const int32_t *gt_idx, *img_off;
  float *loss, *loss_inst, *d_proto, *d_coef;
  float *ws_dc, *ws_l, *ws_wl;  // [ntiles][N][32], [ntiles][N], [N]
  int B, mh, mw, npix, N, G, crop, roi_norm, cap, ntiles, want_dc;
  float alpha;
};

// roi_norm applied to a pixel sum in the reference's order: / (b2 - b0) mw / (b3 - b1) mh * (crop ? mh mw : 1)
__device__ __forceinline__ float roi_normalise(const MlParams &p, const float *b4, float v) {
  if (!p.roi_norm) return v;
  const float gw = (b4[2] - b4[0]) * (float)p.mw, gh = (b4[3] - b4[1]) * (float)p.mh;
  const float wt = p.crop ? (float)(p.mh * p.mw) : 1.f;
  return v / gw / gh * wt;
}

// d loss / d L_j
__device__ __forceinline__ float inst_scale(const MlParams &p, int j) {
  return roi_normalise(p, p.box + (size_t)j * 4, p.weight[j]) * p.alpha / (float)p.mh / (float)p.mw;
}

struct MlTerm {
  static constexpr int STAGED = 2, TAIL = 4 * JC;
  const MlParams &p;
  float *scl;                   // [cap]     d loss / d L_j
  int *grow;                    // [cap]     GT row
  float *redl;                  // [4][JC]   per-wave sums of l
  bool tgt;
  float l;
  __device__ __forceinline__ MlTerm(const MlParams &p_, float *staged, float *tail)
      : p(p_), scl(staged), grow(reinterpret_cast<int *>(staged + p_.cap)), redl(tail) {}
  __device__ __forceinline__ bool crop() const { return p.crop != 0; }
  __device__ __forceinline__ void stage(int i, int j) {
    scl[i] = inst_scale(p, j);
    grow[i] = ymi_clamp_row(p.gt_idx[j], p.G);
  }
  // outside the window q = 0: a GT pixel costs the clamp, the rest nothing
  __device__ __forceinline__ void pixel(int jj, int pix, bool ok) {
    tgt = ok && p.gt[(size_t)grow[jj] * p.npix + pix] != 0;
    l = tgt ? 100.f : 0.f;
  }
  __device__ __forceinline__ float grad(float x, const ymi_sigmoid &s, int, int) {
    const float z = tgt ? -x : x;
    l = fminf(fmaxf(z, 0.f) + log1pf(s.e), 100.f);
    return tgt ? -s.om : s.p;
  }
  __device__ __forceinline__ float mult(float g, int jj) const { return g * scl[jj]; }
  __device__ __forceinline__ void instance_end(int u) {
    l = ymi_wave_sum(l);
    if ((threadIdx.x & 63) == 0) redl[(threadIdx.x >> 6) * JC + u] = l;
  }
  __device__ __forceinline__ void combine(size_t row, int u) const {
    p.ws_l[row] = ((redl[0 * JC + u] + redl[1 * JC + u]) + redl[2 * JC + u]) + redl[3 * JC + u];
  }
};

__global__ __launch_bounds__(256) void mask_loss_k(const MlParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  ymi_lincomb_bwd<MlTerm>(p, lds);
}

// thread = (instance j, channel k): the tile partials in tile order
__global__ __launch_bounds__(256) void mask_loss_dcoef_k(const MlParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)p.N * 32) return;
  const int j = (int)(i >> 5), k = (int)(i & 31);
  if (p.d_coef) p.d_coef[i] = ymi_chunk_sum(p.ws_dc, (size_t)p.N * 32, p.ntiles, i) * inst_scale(p, j);
  if (k == 0) {
    const float L = roi_normalise(p, p.box + (size_t)j * 4, ymi_chunk_sum(p.ws_l, p.N, p.ntiles, j));
    if (p.loss_inst) p.loss_inst[j] = L;
    p.ws_wl[j] = L * p.weight[j];
  }
}

// one block: loss = sum_j weight_j L_j * alpha / mh / mw, strided partial sums then a fixed tree
__global__ __launch_bounds__(256) void mask_loss_sum_k(const MlParams p) {
  const float s = ymi_sum256(p.ws_wl, p.N);
  if (threadIdx.x == 0) p.loss[0] = s * p.alpha / (float)p.mh / (float)p.mw;
}

int validate(const ymi_mask_loss_desc *d) {
  if (!d) return YMI_ENULL;
  if (d->K != 32) return YMI_ESHAPE;                 // cfg.mask_dim of every shipped config (data/config.py:691)
  if (d->B < 1 || d->B > 65535 || d->mh < 1 || d->mw < 1 || d->N < 0 || (d->N > 0 && d->G < 1)) return YMI_EARG;
  if ((d->crop != 0 && d->crop != 1) || (d->roi_norm != 0 && d->roi_norm != 1)) return YMI_EARG;
  if ((long)d->mh * d->mw >= (1L << 26) || (long)d->N >= (1L << 24)) return YMI_ESHAPE;
  return YMI_OK;
}

}  // namespace

// Workspace: [ntiles][N][32] + [ntiles][N] + [N] floats (never empty, so that N = 0 still has a buffer to name)
extern "C" int64_t ymi_mask_loss_ws_bytes(const ymi_mask_loss_desc *d) {
  const int rc = validate(d);
  if (rc) return rc;
  return 4 * ((int64_t)d->N * (33 * (int64_t)ymi_lincomb_ntiles(d->mh, d->mw) + 1)) + 256;
}

extern "C" int ymi_mask_loss_f32(const ymi_mask_loss_desc *d, void *stream) {
  const int rc = validate(d);
  if (rc) return rc;
  if (!d->proto || !d->img_off || !d->loss) return YMI_ENULL;
  if (d->N > 0 && (!d->coef || !d->box || !d->gt || !d->gt_idx || !d->weight || !d->ws)) return YMI_ENULL;
  if (((uintptr_t)d->proto | (uintptr_t)d->d_proto | (uintptr_t)d->ws) & 15) return YMI_ESHAPE;

  MlParams p;
  p.proto = d->proto; p.coef = d->coef; p.box = d->box; p.weight = d->weight;
  p.gt = d->gt; p.gt_idx = d->gt_idx; p.img_off = d->img_off;
  p.loss = d->loss; p.loss_inst = d->loss_inst; p.d_proto = d->d_proto; p.d_coef = d->d_coef;
  p.B = d->B; p.mh = d->mh; p.mw = d->mw; p.npix = d->mh * d->mw; p.N = d->N; p.G = d->G;
  p.crop = d->crop; p.roi_norm = d->roi_norm; p.alpha = d->alpha;
  p.ntiles = ymi_lincomb_ntiles(d->mh, d->mw);
  p.want_dc = d->d_coef != nullptr;
  p.ws_dc = static_cast<float *>(d->ws);
  p.ws_l = p.ws_dc + (size_t)p.ntiles * p.N * 32;
  p.ws_wl = p.ws_l + (size_t)p.ntiles * p.N;
  const size_t lds = ymi_lincomb_lds<MlTerm>(d->N, CAP_MAX, p.cap);                                  // <= 52.9 KB

  int rl = YMI_OK;
  if (d->N > 0 || d->d_proto)                        // (N = 0: the launch only writes the zeros of d_proto)
    rl = ymi_launch(mask_loss_k, dim3(p.ntiles, d->B), dim3(256), lds, stream, p);
  if (!rl && d->N > 0) rl = ymi_launch(mask_loss_dcoef_k, dim3((int)(((long)d->N * 32 + 255) / 256)), dim3(256), 0, stream, p);
  if (!rl) rl = ymi_launch(mask_loss_sum_k, dim3(1), dim3(256), 0, stream, p);
  return rl;
}
