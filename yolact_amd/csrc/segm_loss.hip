// The semantic segmentation term 'S' of MultiBoxLoss (layers/modules/multibox_loss.py:218-239), loss and gradient for a whole
// batch.  The reference loops over the objects of every image in Python around torch.max to build a [K,mh,mw] target; here no
// target tensor exists:
//
// sg_loss_k   grid (pixel tiles, images), one thread = one pixel.  The thread ORs its pixel of every GT mask of the image into a
//             bitset of the K <= 128 classes (four 32-bit words in registers; the labels pass through LDS in chunks of OC, any
//             number of objects), then walks the K channels of segm - for a fixed channel the wave reads consecutive pixels - and
//             takes BCE-with-logits in its stable form max(x, 0) - x t + log1p(exp(-|x|)) and d = scale (sigmoid(x) - t).
// sg_sum_k    one block: the loss from the per-tile partials in a fixed order.
//
// No atomics: the same inputs give the same bits.  A label outside 0 .. K-1 sets no bit and makes the loss NaN.
// Bound by memory traffic: segm is read once and d_segm written once.
#include "loss_common.h"
#include "../../include/yolact_amd.h"

#pragma clang fp contract(off)

namespace {

constexpr int TP = 256;      // pixels per tile (one per thread)
constexpr int OC = 64;       // object labels staged in LDS at once

struct SgParams {
  const float *segm;
  const uint8_t *gt;
  const int32_t *label, *gt_off;
  float *loss, *d_segm, *ws;           // ws [B][ntiles]
  int B, K, HW, G, ntiles;
  float scale;                         // alpha / (mh mw)
};

__global__ __launch_bounds__(TP) void sg_loss_k(const SgParams p) {
  __shared__ int lab[OC];
  __shared__ float lw[TP / 64];
  const int t = threadIdx.x, b = blockIdx.y;
  const int pix = blockIdx.x * TP + t;
  const bool ok = pix < p.HW;
  int g0, n;
  ymi_image_range(p.gt_off, b, p.G, g0, n);

  unsigned w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;
  bool bad = false;
  for (int c0 = 0; c0 < n; c0 += OC) {
    const int cnt = n - c0 < OC ? n - c0 : OC;
    __syncthreads();                                   // the previous chunk has been read
    if (t < cnt) lab[t] = p.label[g0 + c0 + t];
    __syncthreads();
    for (int u = 0; u < cnt; ++u) {
      const int c = lab[u];
      if (c < 0 || c >= p.K) { bad = true; continue; }
      const bool on = ok && p.gt[(size_t)(g0 + c0 + u) * p.HW + pix] != 0;
      const unsigned bit = on ? 1u << (c & 31) : 0u;
      const int word = c >> 5;
      w0 |= word == 0 ? bit : 0u; w1 |= word == 1 ? bit : 0u; w2 |= word == 2 ? bit : 0u; w3 |= word == 3 ? bit : 0u;
    }
  }

  float l = 0.f;
  if (ok) {
    const size_t base = (size_t)b * p.K * p.HW + pix;
    for (int c = 0; c < p.K; ++c) {
      const unsigned w = c < 64 ? (c < 32 ? w0 : w1) : (c < 96 ? w2 : w3);
      const float tg = (w >> (c & 31)) & 1u ? 1.f : 0.f;
      const float x = p.segm[base + (size_t)c * p.HW];
      const float e = expf(-fabsf(x));
      l += (fmaxf(x, 0.f) - x * tg) + log1pf(e);
      if (p.d_segm) {
        const float sg = (x >= 0.f ? 1.f : e) / (1.f + e);
        p.d_segm[base + (size_t)c * p.HW] = p.scale * (sg - tg);
      }
    }
  }
  if (bad) l = ymi_qnan();
  const float s = ymi_block_sum<TP / 64>(l, lw);
  if (t == 0) p.ws[(size_t)b * p.ntiles + blockIdx.x] = s;
}

// one block: loss = scale * the B * ntiles partials, strided sums then a fixed tree
__global__ __launch_bounds__(256) void sg_sum_k(const SgParams p) {
  const float s = ymi_sum256(p.ws, (long)p.B * p.ntiles);
  if (threadIdx.x == 0) p.loss[0] = s * p.scale;
}

int validate_shape(const ymi_segm_loss_desc *d) {
  if (!d) return YMI_ENULL;
  if (d->B < 1 || d->B > 65535 || d->K < 1 || d->K > 128 || d->mh < 1 || d->mw < 1 || d->G < 0) return YMI_EARG;
  // mh mw + a tile stays below 2^31: the pixel index of a tile's last thread is an int
  if ((int64_t)d->mh * d->mw > ((int64_t)1 << 31) - TP || (int64_t)d->B * d->K * d->mh * d->mw >= ((int64_t)1 << 31)) return YMI_ESHAPE;
  return YMI_OK;
}

int ntiles_of(const ymi_segm_loss_desc *d) { return (int)(((int64_t)d->mh * d->mw + TP - 1) / TP); }

}  // namespace

extern "C" int64_t ymi_segm_loss_ws_bytes(const ymi_segm_loss_desc *d) {
  const int rc = validate_shape(d);
  if (rc) return rc;
  return ymi_ws_part((int64_t)d->B * ntiles_of(d));
}

extern "C" int ymi_segm_loss_f32(const ymi_segm_loss_desc *d, void *stream) {
  const int rc = validate_shape(d);
  if (rc) return rc;
  if (!d->segm || !d->gt_off || !d->gt_off_host || !d->loss || !d->ws) return YMI_ENULL;
  if (d->G > 0 && (!d->gt || !d->label)) return YMI_ENULL;
  if (((uintptr_t)d->segm | (uintptr_t)d->d_segm | (uintptr_t)d->ws) & 15) return YMI_ESHAPE;
  const int ro = ymi_validate_offsets(d->gt_off_host, d->B, d->G, 0, d->G);    // ascending offsets from 0 to G
  if (ro) return ro;

  SgParams p = {};
  p.segm = d->segm; p.gt = d->gt; p.label = d->label; p.gt_off = d->gt_off;
  p.loss = d->loss; p.d_segm = d->d_segm; p.ws = static_cast<float *>(d->ws);
  p.B = d->B; p.K = d->K; p.HW = d->mh * d->mw; p.G = d->G; p.ntiles = ntiles_of(d);
  p.scale = d->alpha / (float)p.HW;
  int rl = ymi_launch(sg_loss_k, dim3(p.ntiles, d->B), dim3(TP), 0, stream, p);
  if (!rl) rl = ymi_launch(sg_sum_k, dim3(1), dim3(256), 0, stream, p);
  return rl;
}
