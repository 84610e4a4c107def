// The lincomb mask loss 'M' of MultiBoxLoss with both gradients in one pass (layers/modules/multibox_loss.py:499-627,650 for the
// switches both shipped base configs train with: crop, emulate-ROI-pooling normalisation, binarised GT, sigmoid; box_utils.py:328-373).
//
//     x = sum_k proto[b,r,c,k] * coef[j,k]     p = sigmoid(x)     q = inside_j(r,c) ? p : 0     l = BCE(q, t)
//     L_j = sum_{r,c} l  (roi_norm: / box width in pixels / box height in pixels * (crop ? mh*mw : 1))
//     loss = alpha / mh / mw * sum_j weight_j * L_j                  dl/dx = inside ? p - t : 0
//
// mask_loss_k: grid (pixel tiles, images), 256 threads, one thread = one pixel of a 256-pixel tile.  The pixel's 32 prototype values
// and its 32 d_proto accumulators live in registers for the whole launch; the image's coefficient rows, crop windows, scales and
// GT rows are staged in LDS (up to CAP_MAX = 320 instances at once, more in further rounds) and read as broadcasts.  A logit is
// consumed where it is produced: nothing of size mh*mw*n exists.  Per instance a wave reduces its 64 values of l and of
// g * proto[k] (a register transpose-reduce: 32 shuffles for the 32 channels, lane 2k ends up with channel k), the four waves are
// combined in a fixed order through LDS every JC instances, and the tile's partial goes to the workspace.  A wave none of whose
// pixels lies inside the instance's crop window skips the dot product, exp and log (g = 0, l = 100 t there).
// mask_loss_dcoef_k sums the tile partials in tile order (d_coef, L_j); mask_loss_sum_k sums weight_j * L_j in a fixed tree.
// No floating-point atomics anywhere: the same inputs give the same bits.
//
// Numerics.  With e = exp(-|x|), r = 1 / (1 + e): p = r or e r, 1 - p = e r or r (no cancellation), and the inside-window BCE is
// softplus(-+x) = max(-+x, 0) + log1p(e), capped at the reference's 100.  For |x| <= 12 this is the reference's
// -max(log q, -100) to fp32 round-off (and closer to the exact value than log(1 - p) of a rounded p).  Beyond |x| ~ 17 the
// reference's fp32 sigmoid saturates to exactly 0 or 1, its BCE jumps to the clamp 100 and its gradient to 0; this kernel stays on
// the smooth branch there: l = min(softplus, 100), g = p - t.  Everything stays finite for any finite input.
#include "loss_common.h"
#include "../../include/yolact_amd.h"

namespace {

constexpr int TP = 256;         // pixels per block (one per thread)
constexpr int JC = 8;           // instances between two cross-wave combines: JC * 32 = 256 sums, one per thread
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

__global__ __launch_bounds__(256) void mask_loss_k(const MlParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *cs = lds;                                   // [cap][32] coefficient rows
  float *win = cs + p.cap * 32;                      // [cap][4]  crop window x1, x2, y1, y2
  float *scl = win + p.cap * 4;                      // [cap]     d loss / d L_j
  int *grow = reinterpret_cast<int *>(scl + p.cap);  // [cap]     GT row
  float *red = reinterpret_cast<float *>(grow + p.cap);   // [4][JC][32] per-wave sums of g * proto[k]
  float *redl = red + 4 * JC * 32;                   // [4][JC]   per-wave sums of l

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.y, tile = blockIdx.x;
  const int pix = tile * TP + t;
  const bool ok = pix < p.npix;
  const int py = ok ? pix / p.mw : 0, px = ok ? pix - py * p.mw : 0;
  const float fx = (float)px, fy = (float)py;

  int j0, nj;
  ymi_image_range(p.img_off, b, p.N, j0, nj);
  const int j1 = j0 + nj;

  float P[32], dp[32];
  {
    const float *src = p.proto + ((size_t)b * p.npix + (ok ? pix : 0)) * 32;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(src + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) { P[4 * q + e] = ok ? v[e] : 0.f; dp[4 * q + e] = 0.f; }
    }
  }

  for (int c0 = j0; c0 < j1; c0 += p.cap) {
    const int cnt = j1 - c0 < p.cap ? j1 - c0 : p.cap;
    __syncthreads();                                 // the previous round's rows have been read
    for (int i = t; i < cnt * 32; i += 256) cs[i] = p.coef[(size_t)c0 * 32 + i];
    for (int i = t; i < cnt; i += 256) {
      const int j = c0 + i;
      const float *b4 = p.box + (size_t)j * 4;
      float x1 = 0.f, x2 = (float)p.mw, y1 = 0.f, y2 = (float)p.mh;
      if (p.crop) {
        // sanitize_coordinates(_x1, _x2, img_size, padding=1, cast=False)
        const float a = b4[0] * (float)p.mw, c = b4[2] * (float)p.mw;
        x1 = fminf(a, c) - 1.f; x1 = x1 < 0.f ? 0.f : x1;
        x2 = fmaxf(a, c) + 1.f; x2 = x2 > (float)p.mw ? (float)p.mw : x2;
        const float d = b4[1] * (float)p.mh, e = b4[3] * (float)p.mh;
        y1 = fminf(d, e) - 1.f; y1 = y1 < 0.f ? 0.f : y1;
        y2 = fmaxf(d, e) + 1.f; y2 = y2 > (float)p.mh ? (float)p.mh : y2;
      }
      win[4 * i + 0] = x1; win[4 * i + 1] = x2; win[4 * i + 2] = y1; win[4 * i + 3] = y2;
      scl[i] = inst_scale(p, j);
      int g = p.gt_idx[j];
      grow[i] = g < 0 ? 0 : (g >= p.G ? p.G - 1 : g);
    }
    __syncthreads();

    for (int jj0 = 0; jj0 < cnt; jj0 += JC) {
#pragma unroll 1
      for (int u = 0; u < JC; ++u) {
        const int jj = jj0 + u;
        if (jj >= cnt) break;                        // block-uniform
        const float *c = cs + jj * 32;
        const f32x4 w4 = *reinterpret_cast<const f32x4 *>(win + 4 * jj);
        const bool tgt = ok && p.gt[(size_t)grow[jj] * p.npix + pix] != 0;
        const bool inside = ok && fx >= w4[0] && fx < w4[1] && fy >= w4[2] && fy < w4[3];
        float l = tgt ? 100.f : 0.f, g = 0.f;        // outside the window q = 0: a GT pixel costs the clamp, the rest nothing
        const bool any_in = __any(inside) != 0;      // wave-uniform
        if (any_in) {
          float x = 0.f;
#pragma unroll
          for (int k = 0; k < 32; ++k) x = fmaf(P[k], c[k], x);
          const float e = expf(-fabsf(x));
          const float r = 1.f / (1.f + e), er = e * r;
          const float pr = x >= 0.f ? r : er, om = x >= 0.f ? er : r;      // p, 1 - p
          if (inside) {
            const float z = tgt ? -x : x;
            l = fminf(fmaxf(z, 0.f) + log1pf(e), 100.f);
            g = tgt ? -om : pr;
          }
          const float gs = g * scl[jj];
#pragma unroll
          for (int k = 0; k < 32; ++k) dp[k] = fmaf(gs, c[k], dp[k]);
        }
        l = ymi_wave_sum(l);
        if (lane == 0) redl[wave * JC + u] = l;
        if (p.want_dc) {
          float v0 = 0.f;
          if (any_in) {
            // transpose-reduce of v[k] = g * P[k] over the wave: at distance m = 32, 16, .., 2 a lane keeps the upper or the
            // lower half of its values (by its bit m) and receives the partner's sums of that half; after five steps lane l
            // holds channel l >> 1 summed over the 32 lanes that share its bit 0, the last step adds the other 32
            float v[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) v[k] = g * P[k];
#pragma unroll
            for (int s = 0; s < 5; ++s) {
              const int half = 16 >> s, m = 32 >> s;
              const bool up = (lane & m) != 0;
#pragma unroll
              for (int i = 0; i < half; ++i) {
                const float keep = up ? v[i + half] : v[i];
                const float send = up ? v[i] : v[i + half];
                v[i] = keep + __shfl_xor(send, m);
              }
            }
            v0 = v[0] + __shfl_xor(v[0], 1);
          }
          if (!(lane & 1)) red[(wave * JC + u) * 32 + (lane >> 1)] = v0;
        }
      }
      __syncthreads();
      {
        // thread = (instance u, channel k): the four waves in order, then the tile's partial
        const int u = t >> 5, k = t & 31, jj = jj0 + u;
        if (jj < cnt) {
          const size_t row = (size_t)tile * p.N + (c0 + jj);
          // ymi_waves_sum's order, spelled out: through the helper the compiler pairs these LDS reads differently
          if (p.want_dc)
            p.ws_dc[row * 32 + k] = ((red[(0 * JC + u) * 32 + k] + red[(1 * JC + u) * 32 + k]) + red[(2 * JC + u) * 32 + k]) +
                                    red[(3 * JC + u) * 32 + k];
          if (k == 0) p.ws_l[row] = ((redl[0 * JC + u] + redl[1 * JC + u]) + redl[2 * JC + u]) + redl[3 * JC + u];
        }
      }
      __syncthreads();
    }
  }

  if (p.d_proto && ok) {
    float *dst = p.d_proto + ((size_t)b * p.npix + pix) * 32;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = dp[4 * q + e];
      *reinterpret_cast<f32x4 *>(dst + 4 * q) = v;
    }
  }
}

// thread = (instance j, channel k): the tile partials in tile order
__global__ __launch_bounds__(256) void mask_loss_dcoef_k(const MlParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)p.N * 32) return;
  const int j = (int)(i >> 5), k = (int)(i & 31);
  if (p.d_coef) {
    float s = 0.f;
    for (int tl = 0; tl < p.ntiles; ++tl) s += p.ws_dc[((size_t)tl * p.N + j) * 32 + k];
    p.d_coef[i] = s * inst_scale(p, j);
  }
  if (k == 0) {
    float s = 0.f;
    for (int tl = 0; tl < p.ntiles; ++tl) s += p.ws_l[(size_t)tl * p.N + j];
    const float L = roi_normalise(p, p.box + (size_t)j * 4, s);
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

int ntiles_of(const ymi_mask_loss_desc *d) { return (d->mh * d->mw + TP - 1) / TP; }

}  // namespace

// Workspace: [ntiles][N][32] + [ntiles][N] + [N] floats (never empty, so that N = 0 still has a buffer to name)
extern "C" int64_t ymi_mask_loss_ws_bytes(const ymi_mask_loss_desc *d) {
  const int rc = validate(d);
  if (rc) return rc;
  return 4 * ((int64_t)d->N * (33 * (int64_t)ntiles_of(d) + 1)) + 256;
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
  p.ntiles = ntiles_of(d);
  p.want_dc = d->d_coef != nullptr;
  p.ws_dc = static_cast<float *>(d->ws);
  p.ws_l = p.ws_dc + (size_t)p.ntiles * p.N * 32;
  p.ws_wl = p.ws_l + (size_t)p.ntiles * p.N;
  const int n8 = (d->N + 7) / 8 * 8;
  p.cap = n8 < 8 ? 8 : (n8 > CAP_MAX ? CAP_MAX : n8);
  const size_t lds = ((size_t)p.cap * (32 + 4 + 1 + 1) + 4 * JC * 32 + 4 * JC) * sizeof(float);     // <= 52.9 KB

  int rl = YMI_OK;
  if (d->N > 0 || d->d_proto)                        // (N = 0: the launch only writes the zeros of d_proto)
    rl = ymi_launch(mask_loss_k, dim3(p.ntiles, d->B), dim3(256), lds, stream, p);
  if (!rl && d->N > 0) rl = ymi_launch(mask_loss_dcoef_k, dim3((int)(((long)d->N * 32 + 255) / 256)), dim3(256), 0, stream, p);
  if (!rl) rl = ymi_launch(mask_loss_sum_k, dim3(1), dim3(256), 0, stream, p);
  return rl;
}
