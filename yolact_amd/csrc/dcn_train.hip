// The train path's deformable convolution (layers/train_ops.py deform_conv): the reference's own im2col + GEMM split
// (external/DCNv2/src/cuda/dcn_v2_cuda.cu:42-335) with the GEMM left to the existing bit-reproducible convolution kernels and the
// column tensor's two directions here.  Geometry: 3x3, padding 1, dilation 1, one deformable group, square stride 1 or 2, NHWC fp32,
// Cin % 32 == 0.  om [B,Ho,Wo,27]: channel 2k = dh_k, 2k + 1 = dw_k, 18 + k = the mask LOGIT of tap k = 3i + j.
//
// Notation: m = output pixel (b, oy, ox), item = m * 9 + k, sample point (h, w) = (oy*s - 1 + i) + dh_k, (ox*s - 1 + j) + dw_k formed
// in fp32 as csrc/dcn.hip and dcn_bwd.hip::dcn_point form it, mu_k = 1 / (1 + expf(-logit_k)), S_k[c] the zero-padded bilinear sample
// of x[b, :, :, c] at the point.  col is [B,Ho,Wo,9*Cin] = [item][Cin].
//     col[item, c]  = ((uh*uw) v0 + (uh*lw) v1 + (lh*uw) v2 + (lh*lw) v3) * mu        (dcn_bwd.hip's column tile, the same roundings)
//     g_dh[m,k]     = mu * sum_c dcol[item,c] * dS[c]/dh     (g_dw likewise; at an integer coordinate the derivative of the cell
//                     [h, h + 1], as dcn_point has it), g_logit[m,k] = mu (1 - mu) * sum_c dcol[item,c] * S[c]; all three exactly 0.0
//                     for a point outside -1 < h < H, -1 < w < W
//     gx[t,c]       = sum over the entries (item, corner) whose corner is pixel t of (corner weight * mu) * dcol[item,c]
//
// NO floating-point atomic and no sum whose order depends on which block or wave arrives first:
//   * cols_fwd_k / cols_om_k: eight lanes own one item and walk its channels 32 at a time, four per lane (one 16-byte load per corner,
//     128 contiguous bytes per item and instruction); the geometry is formed once per item, before the channel loop, in the lanes
//     that use it.  The three dot products of cols_om_k are summed per lane in channel order (chunk ascending, the four elements of a
//     load ascending) and then over the eight lanes by the butterfly 4, 2, 1: one fixed tree, a function of Cin alone.
//   * gx is a GATHER over an inverted index, not a scatter.  cols_entries_k writes, per (item, corner), the target pixel
//     t = (b*H + y)*W + x (B*H*W for a corner outside the image or a gated-out point) and the coefficient.  The caller sorts the keys
//     STABLY (any stable sort gives the same permutation: ascending t, ties in entry order).  seg_starts_k finds by bisection where
//     each pixel's run begins, and cols_gx_k gives every (pixel, four channels) to one thread that walks the run front to back from
//     +0.0.  The order of a pixel's additions is therefore canonical: ascending (m, tap, corner).  A pixel nobody samples gets +0.0.
//     Every index read from the sorted list is bounded against the entry count 36 * B*Ho*Wo before it is used (a wrong permutation
//     gives wrong sums, never an access outside dcol or coef), and every run against [0, entry count].
#include "loss_common.h"
#include "../../include/yolact_amd.h"

namespace {

struct ColsParams {
  const float *x, *om, *dcol, *coef_in;
  float *col, *g_om, *gx, *coef;
  int32_t *keys, *seg;
  const int32_t *skeys;
  const int64_t *order;
  int B, H, W, Cin, Ho, Wo, stride;
  int M, HoWo, NP;              // output pixels, Ho*Wo, input pixels B*H*W
  long items, entries;          // 9 M, 36 M
};

// One sample point (dcn_bwd.hip's dcn_point with the logit's sigmoid): pixel index of its top-left corner (meaningful only for
// corners whose bit is set), which corners (bit 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right) lie inside the image — none
// when the point is gated out — the fractions and the modulation.
struct Pt { int t1; unsigned fl; float lh, lw, mk; };

__device__ __forceinline__ Pt tr_point(const ColsParams &p, long item) {
  Pt g;
  const int m = (int)(item / 9), tap = (int)(item - (long)m * 9);
  const int b = m / p.HoWo, pix = m - b * p.HoWo;
  const int oy = pix / p.Wo, ox = pix - oy * p.Wo;
  const float *om = p.om + (size_t)m * 27;
  const float dh = om[2 * tap], dw = om[2 * tap + 1];
  g.mk = 1.f / (1.f + expf(-om[18 + tap]));
  g.t1 = 0; g.fl = 0u; g.lh = 0.f; g.lw = 0.f;
  const int ky = tap / 3, kx = tap - 3 * ky;
  const float h = (float)(oy * p.stride - 1 + ky) + dh, w = (float)(ox * p.stride - 1 + kx) + dw;
  const bool in = h > -1.f && w > -1.f && h < (float)p.H && w < (float)p.W;
  if (!in) return g;
  const int hl = (int)floorf(h), wl = (int)floorf(w);
  g.lh = h - (float)hl; g.lw = w - (float)wl;
  g.t1 = (b * p.H + hl) * p.W + wl;
  const bool t_ = hl >= 0, b_ = hl + 1 <= p.H - 1, l_ = wl >= 0, r_ = wl + 1 <= p.W - 1;
  g.fl = (unsigned)(t_ && l_) | ((unsigned)(t_ && r_) << 1) | ((unsigned)(b_ && l_) << 2) | ((unsigned)(b_ && r_) << 3);
  return g;
}

// the four corners' channels [c, c + 4) of a point, zeros for corners outside the image
struct Corners { f32x4 v0, v1, v2, v3; };
__device__ __forceinline__ Corners tr_corners(const ColsParams &p, const Pt &g, int c) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  // (t1 may be negative for a point whose top or left corners lie outside: the products below are formed in 64 bits and only the
  // corners whose bit is set are dereferenced)
  const float *xb = p.x + (long)g.t1 * p.Cin + c;
  const long dx = p.Cin, dy = (long)p.W * p.Cin;
  Corners k;
  k.v0 = (g.fl & 1u) ? *reinterpret_cast<const f32x4 *>(xb) : z;
  k.v1 = (g.fl & 2u) ? *reinterpret_cast<const f32x4 *>(xb + dx) : z;
  k.v2 = (g.fl & 4u) ? *reinterpret_cast<const f32x4 *>(xb + dy) : z;
  k.v3 = (g.fl & 8u) ? *reinterpret_cast<const f32x4 *>(xb + dy + dx) : z;
  return k;
}

// eight lanes per item: 32 items per 256-thread block
__global__ __launch_bounds__(256) void cols_fwd_k(const ColsParams p) {
  const long item = (long)blockIdx.x * 32 + (threadIdx.x >> 3);
  if (item >= p.items) return;
  const int l8 = threadIdx.x & 7;
  const Pt g = tr_point(p, item);
  const float uh = 1.f - g.lh, uw = 1.f - g.lw;
  const float w0 = uh * uw, w1 = uh * g.lw, w2 = g.lh * uw, w3 = g.lh * g.lw;
  float *dst = p.col + (size_t)item * p.Cin;
  for (int c = 4 * l8; c < p.Cin; c += 32) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (g.fl) {
      const Corners k = tr_corners(p, g, c);
      v = (w0 * k.v0 + w1 * k.v1 + w2 * k.v2 + w3 * k.v3) * g.mk;
    }
    *reinterpret_cast<f32x4 *>(dst + c) = v;
  }
}

__global__ __launch_bounds__(256) void cols_om_k(const ColsParams p) {
  long item = (long)blockIdx.x * 32 + (threadIdx.x >> 3);
  const bool live = item < p.items;
  if (!live) item = p.items - 1;                         // (every lane reaches the butterfly)
  const int l8 = threadIdx.x & 7;
  const Pt g = tr_point(p, item);
  const float uh = 1.f - g.lh, uw = 1.f - g.lw;
  const float w0 = uh * uw, w1 = uh * g.lw, w2 = g.lh * uw, w3 = g.lh * g.lw;
  float sm = 0.f, sh = 0.f, sw = 0.f;
  if (g.fl) {
    const float *src = p.dcol + (size_t)item * p.Cin;
    for (int c = 4 * l8; c < p.Cin; c += 32) {
      const Corners k = tr_corners(p, g, c);
      const f32x4 d = *reinterpret_cast<const f32x4 *>(src + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float S = w0 * k.v0[e] + w1 * k.v1[e] + w2 * k.v2[e] + w3 * k.v3[e];
        sm += d[e] * S;
        sh += d[e] * (uw * (k.v2[e] - k.v0[e]) + g.lw * (k.v3[e] - k.v1[e]));
        sw += d[e] * (uh * (k.v1[e] - k.v0[e]) + g.lh * (k.v3[e] - k.v2[e]));
      }
    }
  }
#pragma unroll
  for (int d = 4; d >= 1; d >>= 1) {
    sm += __shfl_xor(sm, d);
    sh += __shfl_xor(sh, d);
    sw += __shfl_xor(sw, d);
  }
  if (live && l8 == 0) {
    const int m = (int)(item / 9), tap = (int)(item - (long)m * 9);
    float *o = p.g_om + (size_t)m * 27;
    const bool on = g.fl != 0u;
    o[2 * tap] = on ? g.mk * sh : 0.f;
    o[2 * tap + 1] = on ? g.mk * sw : 0.f;
    o[18 + tap] = on ? (g.mk * (1.f - g.mk)) * sm : 0.f;
  }
}

// one thread per item: its four entries (target pixel or the sentinel NP, coefficient), 16-byte stores
__global__ __launch_bounds__(256) void cols_entries_k(const ColsParams p) {
  const long item = (long)blockIdx.x * 256 + threadIdx.x;
  if (item >= p.items) return;
  const Pt g = tr_point(p, item);
  const float uh = 1.f - g.lh, uw = 1.f - g.lw;
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  i32x4 key;
  key[0] = (g.fl & 1u) ? g.t1 : p.NP;
  key[1] = (g.fl & 2u) ? g.t1 + 1 : p.NP;
  key[2] = (g.fl & 4u) ? g.t1 + p.W : p.NP;
  key[3] = (g.fl & 8u) ? g.t1 + p.W + 1 : p.NP;
  f32x4 cf;
  cf[0] = (g.fl & 1u) ? (uh * uw) * g.mk : 0.f;
  cf[1] = (g.fl & 2u) ? (uh * g.lw) * g.mk : 0.f;
  cf[2] = (g.fl & 4u) ? (g.lh * uw) * g.mk : 0.f;
  cf[3] = (g.fl & 8u) ? (g.lh * g.lw) * g.mk : 0.f;
  *reinterpret_cast<i32x4 *>(p.keys + 4 * item) = key;
  *reinterpret_cast<f32x4 *>(p.coef + 4 * item) = cf;
}

// seg[t] = the first position of the sorted keys that holds a key >= t, t = 0 .. NP (bisection: at most 32 steps, every probe
// inside [0, entries))
__global__ __launch_bounds__(256) void seg_starts_k(const ColsParams p) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t > p.NP) return;
  long lo = 0, hi = p.entries;
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if (p.skeys[mid] < (int)t) lo = mid + 1; else hi = mid;
  }
  p.seg[t] = (int)lo;
}

// one thread per (input pixel, four channels): the pixel's run of the sorted list, front to back, four entries in flight
__global__ __launch_bounds__(256) void cols_gx_k(const ColsParams p) {
  const int c4n = p.Cin >> 2;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long t = gid / c4n;
  if (t >= p.NP) return;
  const int c = (int)(gid - t * c4n) * 4;
  long s0 = p.seg[t], s1 = p.seg[t + 1];
  s0 = s0 < 0 ? 0 : (s0 > p.entries ? p.entries : s0);
  s1 = s1 < s0 ? s0 : (s1 > p.entries ? p.entries : s1);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (long i = s0; i < s1; i += 4) {
    long e[4];
    float cf[4];
    f32x4 d[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) e[u] = i + u < s1 ? p.order[i + u] : -1;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool ok = e[u] >= 0 && e[u] < p.entries;     // (an entry is (item, corner): item = e >> 2 < 9 M)
      cf[u] = ok ? p.coef_in[e[u]] : 0.f;
      d[u] = ok ? *reinterpret_cast<const f32x4 *>(p.dcol + (size_t)(e[u] >> 2) * p.Cin + c) : z;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + u < s1) acc += cf[u] * d[u];
  }
  *reinterpret_cast<f32x4 *>(p.gx + (size_t)t * p.Cin + c) = acc;
}

int cols_validate(const ymi_dcn_cols_desc *d, ColsParams &p) {
  if (!d) return YMI_ENULL;
  if (d->B < 1 || d->H < 1 || d->W < 1 || d->Cin < 1) return YMI_EARG;
  if (d->stride != 1 && d->stride != 2) return YMI_EARG;
  if (d->Cin % 32 != 0) return YMI_ESHAPE;
  if (d->Ho != (d->H + 2 - 3) / d->stride + 1 || d->Wo != (d->W + 2 - 3) / d->stride + 1 || d->Ho < 1 || d->Wo < 1) return YMI_ESHAPE;
  const long M = (long)d->B * d->Ho * d->Wo, NP = (long)d->B * d->H * d->W;
  const long lim = 1L << 31;
  if (NP * d->Cin >= lim || M * 9 * d->Cin >= lim || M * 27 >= lim || M * 36 >= lim) return YMI_ESHAPE;
  p.x = d->x; p.om = d->om; p.dcol = d->dcol; p.coef_in = d->coef;
  p.col = d->col; p.g_om = d->g_om; p.gx = d->gx; p.coef = d->coef;
  p.keys = d->keys; p.seg = d->seg; p.skeys = d->sorted_keys; p.order = d->order;
  p.B = d->B; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.Ho = d->Ho; p.Wo = d->Wo; p.stride = d->stride;
  p.M = (int)M; p.HoWo = d->Ho * d->Wo; p.NP = (int)NP;
  p.items = 9 * M; p.entries = 36 * M;
  return YMI_OK;
}

inline bool misaligned16(const void *a, const void *b = nullptr, const void *c = nullptr, const void *e = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)e) & 15) != 0;
}

}  // namespace

extern "C" int ymi_dcn_cols_fwd_f32(const ymi_dcn_cols_desc *d, void *stream) {
  ColsParams p;
  const int rc = cols_validate(d, p);
  if (rc) return rc;
  if (!d->x || !d->om || !d->col) return YMI_ENULL;
  if (misaligned16(d->x, d->col)) return YMI_ESHAPE;
  return ymi_launch(cols_fwd_k, dim3((unsigned)((p.items + 31) / 32)), dim3(256), 0, stream, p);
}

extern "C" int ymi_dcn_cols_entries_f32(const ymi_dcn_cols_desc *d, void *stream) {
  ColsParams p;
  const int rc = cols_validate(d, p);
  if (rc) return rc;
  if (!d->om || !d->keys || !d->coef) return YMI_ENULL;
  if (misaligned16(d->keys, d->coef)) return YMI_ESHAPE;
  return ymi_launch(cols_entries_k, dim3((unsigned)((p.items + 255) / 256)), dim3(256), 0, stream, p);
}

extern "C" int ymi_dcn_cols_bwd_f32(const ymi_dcn_cols_desc *d, void *stream) {
  ColsParams p;
  int rc = cols_validate(d, p);
  if (rc) return rc;
  if (!d->g_om && !d->gx) return YMI_OK;
  if (!d->dcol) return YMI_ENULL;
  if (d->g_om && (!d->x || !d->om)) return YMI_ENULL;
  if (d->gx && (!d->sorted_keys || !d->order || !d->coef || !d->seg)) return YMI_ENULL;
  if (misaligned16(d->dcol, d->x, d->gx)) return YMI_ESHAPE;
  if (d->g_om) rc = ymi_launch(cols_om_k, dim3((unsigned)((p.items + 31) / 32)), dim3(256), 0, stream, p);
  if (!rc && d->gx) {
    rc = ymi_launch(seg_starts_k, dim3((unsigned)(((long)p.NP + 1 + 255) / 256)), dim3(256), 0, stream, p);
    const long threads = (long)p.NP * (p.Cin >> 2);
    if (!rc) rc = ymi_launch(cols_gx_k, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, p);
  }
  return rc;
}
