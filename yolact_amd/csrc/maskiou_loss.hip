// The mask-IoU term 'I' of YOLACT++ (layers/modules/multibox_loss.py:629-672, 684-694): everything around FastMaskIoUNet's forward
// that training needs, in fp32, without floating-point atomics (the same inputs give the same bits).
//
//   ymi_maskiou_input_f32       x0[j] = inside_j ? sigmoid(proto[b] . coef[j]) : 0 (the net's input) and iou_t[j] = inter / (a1 + a2 -
//                               inter) from three integer counts.  One block per instance; a thread walks the pixels t, t + 256, ..
//                               and evaluates the logit only inside the crop window (ymi_crop_window: padding 1).
//   ymi_maskiou_input_bwd_f32   d_proto, d_coef from d_x0: lincomb_common.h's ymi_lincomb_bwd with g = inside ? d_x0 p (1 - p) : 0
//                               supplied from outside; miou_dcoef_k sums the tile partials in tile order.
//   ymi_conv2d_bwd_nhwc_f32     the backward of ymi_conv2d_direct_nhwc_f32 (+ ReLU) for any kernel size, stride and padding:
//                               dx as a gather (an input pixel sums the output pixels that read it, taps in (ky, kx) order, channels
//                               in order; pixels no window reaches get exact zeros); dw and db as dw[k,co] = sum_pos im2col[pos,k]
//                               dy[pos,co] with a row k = K of ones for db: the positions are cut into chunks, a block owns a
//                               (16 RK) x (16 RC) tile of [K + 1, Cout] and one chunk, stages 16 positions at a time in LDS and adds
//                               them in position order; RK, RC in {1, 2, 4} and the chunk count follow the layer's shape (72 weights
//                               over 3.7 M positions and 73 728 weights over 7 200 positions are both one launch of ~1000 blocks);
//                               a second launch adds the chunk partials in chunk order.
//   ymi_global_maxpool_bwd_nhwc_f32   routes d_pool[n,c] to the FIRST maximum of y[n,:,c] in row-major order (torch's CPU max_pool2d).
//   ymi_maskiou_head_f32        p = pool[n,label[n]], loss = alpha sum_n smooth_l1(p - iou_t[n]), d_pool (zero off the label).
#include "lincomb_common.h"
#include "../../include/yolact_amd.h"

namespace {

// ---- the net's input and the IoU targets --------------------------------------------------------------------------------------
constexpr int CAP_MAX = 128;    // instances staged in LDS at once (more take further rounds)

struct MiParams {
  const float *proto, *coef, *box, *d_x0;
  const uint8_t *gt;
  const int32_t *gt_idx, *img_off;
  float *x0, *iou_t, *d_proto, *d_coef, *ws_dc;       // ws_dc [ntiles][N][32]
  int B, mh, mw, npix, N, G, cap, ntiles, want_dc;
};

__global__ __launch_bounds__(256) void miou_input_k(const MiParams p) {
  __shared__ __attribute__((aligned(16))) float cs[32];
  __shared__ int cw[3][4];
  const int j = blockIdx.x, t = threadIdx.x;
  int b = 0;                                         // the last image whose first instance is <= j
  for (int i = 1; i < p.B; ++i) b = p.img_off[i] <= j ? i : b;
  if (t < 32) cs[t] = p.coef[(size_t)j * 32 + t];
  const f32x4 w4 = ymi_crop_window(p.box + (size_t)j * 4, p.mh, p.mw);
  const uint8_t *gt = p.gt + (size_t)ymi_clamp_row(p.gt_idx[j], p.G) * p.npix;
  const float *proto = p.proto + (size_t)b * p.npix * 32;
  float *x0 = p.x0 + (size_t)j * p.npix;
  __syncthreads();
  int a1 = 0, a2 = 0, in = 0;
  for (int pix = t; pix < p.npix; pix += 256) {
    const int py = pix / p.mw, px = pix - py * p.mw;
    const float fx = (float)px, fy = (float)py;
    const bool tgt = gt[pix] != 0;
    const bool inside = ymi_in_window(w4, fx, fy);
    float v = 0.f;
    if (inside) {
      const float *src = proto + (size_t)pix * 32;
      float x = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const f32x4 pv = *reinterpret_cast<const f32x4 *>(src + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) x = fmaf(pv[e], cs[4 * q + e], x);
      }
      v = ymi_sigmoid_split(x).p;
      a1 += x > 0.f;
      in += x > 0.f && tgt;
    }
    a2 += tgt;
    x0[pix] = v;
  }
  a1 = ymi_wave_sum(a1); a2 = ymi_wave_sum(a2); in = ymi_wave_sum(in);
  if ((t & 63) == 0) { cw[0][t >> 6] = a1; cw[1][t >> 6] = a2; cw[2][t >> 6] = in; }
  __syncthreads();
  if (t == 0) {
    const float fa1 = (float)ymi_waves_count<4>(cw[0]), fa2 = (float)ymi_waves_count<4>(cw[1]);
    const float fin = (float)ymi_waves_count<4>(cw[2]);
    p.iou_t[j] = fin / ((fa1 + fa2) - fin);          // _mask_iou's order (:676-682); 0 / 0 is its NaN
  }
}

struct MiTerm {
  static constexpr int STAGED = 0, TAIL = 0;
  const MiParams &p;
  __device__ __forceinline__ MiTerm(const MiParams &p_, float *, float *) : p(p_) {}
  __device__ __forceinline__ bool crop() const { return true; }
  __device__ __forceinline__ void stage(int, int) {}
  __device__ __forceinline__ void pixel(int, int, bool) {}
  __device__ __forceinline__ float grad(float, const ymi_sigmoid &s, int j, int pix) const {
    return p.d_x0[(size_t)j * p.npix + pix] * s.p * s.om;
  }
  __device__ __forceinline__ float mult(float g, int) const { return g; }
  __device__ __forceinline__ void instance_end(int) {}
  __device__ __forceinline__ void combine(size_t, int) const {}
};

__global__ __launch_bounds__(256) void miou_input_bwd_k(const MiParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  ymi_lincomb_bwd<MiTerm>(p, lds);
}

// thread = (instance j, channel k): the tile partials in tile order
__global__ __launch_bounds__(256) void miou_dcoef_k(const MiParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)p.N * 32) return;
  p.d_coef[i] = ymi_chunk_sum(p.ws_dc, (size_t)p.N * 32, p.ntiles, i);
}

int validate_input(const ymi_maskiou_input_desc *d) {
  if (!d) return YMI_ENULL;
  if (d->K != 32) return YMI_ESHAPE;
  if (d->B < 1 || d->B > 65535 || d->mh < 1 || d->mw < 1 || d->N < 1 || d->G < 1) return YMI_EARG;
  if ((long)d->mh * d->mw >= (1L << 24) || (long)d->N >= (1L << 24)) return YMI_ESHAPE;      // the counts stay exact in fp32
  return YMI_OK;
}

int validate_input_ptrs(const ymi_maskiou_input_desc *d) {
  if (!d->proto || !d->coef || !d->box || !d->img_off || !d->img_off_host) return YMI_ENULL;
  if ((uintptr_t)d->proto & 15) return YMI_ESHAPE;
  return ymi_validate_offsets(d->img_off_host, d->B, d->N, 0, d->N);
}

MiParams mi_params(const ymi_maskiou_input_desc *d) {
  MiParams p;
  p.proto = d->proto; p.coef = d->coef; p.box = d->box; p.d_x0 = d->d_x0; p.gt = d->gt; p.gt_idx = d->gt_idx; p.img_off = d->img_off;
  p.x0 = d->x0; p.iou_t = d->iou_t; p.d_proto = d->d_proto; p.d_coef = d->d_coef; p.ws_dc = static_cast<float *>(d->ws);
  p.B = d->B; p.mh = d->mh; p.mw = d->mw; p.npix = d->mh * d->mw; p.N = d->N; p.G = d->G;
  p.ntiles = ymi_lincomb_ntiles(d->mh, d->mw); p.want_dc = d->d_coef != nullptr;
  p.cap = 0;                                         // the backward's (ymi_lincomb_lds)
  return p;
}

// ---- convolution backward ---------------------------------------------------------------------------------------------------------
struct CbParams {
  const float *x, *w, *y, *dy;
  float *dx, *dw, *db, *ws;
  int B, H, W, Cin, Ho, Wo, Cout, ldw, kh, kw, stride, pad, relu;
  int K, nct, nchunks;
  long P, chunk, total;
};

// thread = (input pixel, CT input channels)
template <int CT> __global__ __launch_bounds__(256) void conv_dx_k(const CbParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const int ncg = p.Cin / CT;
  const int cg = (int)(i % ncg);
  long r = i / ncg;
  const long pix = r;
  const int ix = (int)(r % p.W); r /= p.W;
  const int iy = (int)(r % p.H);
  const long n = r / p.H;
  const bool vec = (p.Cout & 3) == 0;
  float acc[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) acc[c] = 0.f;
  for (int ky = 0; ky < p.kh; ++ky) {
    const int ty = iy + p.pad - ky;
    if (ty < 0 || ty % p.stride) continue;
    const int oy = ty / p.stride;
    if (oy >= p.Ho) continue;
    for (int kx = 0; kx < p.kw; ++kx) {
      const int tx = ix + p.pad - kx;
      if (tx < 0 || tx % p.stride) continue;
      const int ox = tx / p.stride;
      if (ox >= p.Wo) continue;
      const size_t o = (size_t)((n * p.Ho + oy) * p.Wo + ox) * p.Cout;
      const float *wp = p.w + ((size_t)(ky * p.kw + kx) * p.Cin + (size_t)cg * CT) * p.ldw;
      if (vec) {
        for (int co = 0; co < p.Cout; co += 4) {
          f32x4 d = *reinterpret_cast<const f32x4 *>(p.dy + o + co);
          if (p.relu) {
            const f32x4 yv = *reinterpret_cast<const f32x4 *>(p.y + o + co);
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = yv[e] > 0.f ? d[e] : 0.f;
          }
#pragma unroll
          for (int c = 0; c < CT; ++c) {
            const f32x4 wv = *reinterpret_cast<const f32x4 *>(wp + (size_t)c * p.ldw + co);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[c] = fmaf(d[e], wv[e], acc[c]);
          }
        }
      } else {
        for (int co = 0; co < p.Cout; ++co) {
          float d = p.dy[o + co];
          if (p.relu && !(p.y[o + co] > 0.f)) d = 0.f;
#pragma unroll
          for (int c = 0; c < CT; ++c) acc[c] = fmaf(d, wp[(size_t)c * p.ldw + co], acc[c]);
        }
      }
    }
  }
  float *dst = p.dx + (size_t)pix * p.Cin + (size_t)cg * CT;
#pragma unroll
  for (int c = 0; c < CT; ++c) dst[c] = acc[c];
}

constexpr int PS = 16;          // positions staged at once

// block = (chunk of positions, tile of [K + 1, Cout]); thread (tk, tc) owns RK x RC sums
template <int RK, int RC> __global__ __launch_bounds__(256) void conv_dw_k(const CbParams p) {
  constexpr int TK = 16 * RK, TC = 16 * RC;
  __shared__ float xs[PS][TK];
  __shared__ float ds[PS][TC];
  const int t = threadIdx.x, tk = t >> 4, tc = t & 15;
  const int k0 = ((int)blockIdx.y / p.nct) * TK, c0 = ((int)blockIdx.y % p.nct) * TC;
  const long pos0 = (long)blockIdx.x * p.chunk;
  const long pos1 = pos0 + p.chunk < p.P ? pos0 + p.chunk : p.P;
  float acc[RK][RC];
#pragma unroll
  for (int a = 0; a < RK; ++a)
#pragma unroll
    for (int c = 0; c < RC; ++c) acc[a][c] = 0.f;

  for (long ps = pos0; ps < pos1; ps += PS) {
    __syncthreads();
    for (int e = t; e < PS * TK; e += 256) {
      const int pp = e / TK, kk = e - pp * TK, k = k0 + kk;
      const long pos = ps + pp;
      float v = 0.f;
      if (pos < pos1 && k <= p.K) {
        if (k == p.K) {
          v = 1.f;                                   // the row of ones: db
        } else {
          const int ci = k % p.Cin, tap = k / p.Cin, kx = tap % p.kw, ky = tap / p.kw;
          const int ox = (int)(pos % p.Wo);
          const long r = pos / p.Wo;
          const int oy = (int)(r % p.Ho);
          const long n = r / p.Ho;
          const int iy = oy * p.stride - p.pad + ky, ix = ox * p.stride - p.pad + kx;
          if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) v = p.x[((size_t)(n * p.H + iy) * p.W + ix) * p.Cin + ci];
        }
      }
      xs[pp][kk] = v;
    }
    for (int e = t; e < PS * TC; e += 256) {
      const int pp = e / TC, cc = e - pp * TC, co = c0 + cc;
      const long pos = ps + pp;
      float v = 0.f;
      if (pos < pos1 && co < p.Cout) {
        v = p.dy[(size_t)pos * p.Cout + co];
        if (p.relu && !(p.y[(size_t)pos * p.Cout + co] > 0.f)) v = 0.f;
      }
      ds[pp][cc] = v;
    }
    __syncthreads();
#pragma unroll
    for (int pp = 0; pp < PS; ++pp) {
      float xr[RK], dr[RC];
#pragma unroll
      for (int a = 0; a < RK; ++a) xr[a] = xs[pp][tk * RK + a];
#pragma unroll
      for (int c = 0; c < RC; ++c) dr[c] = ds[pp][tc * RC + c];
#pragma unroll
      for (int a = 0; a < RK; ++a)
#pragma unroll
        for (int c = 0; c < RC; ++c) acc[a][c] = fmaf(xr[a], dr[c], acc[a][c]);
    }
  }
  float *dst = p.ws + (size_t)blockIdx.x * (p.K + 1) * p.ldw;
#pragma unroll
  for (int a = 0; a < RK; ++a) {
    const int k = k0 + tk * RK + a;
#pragma unroll
    for (int c = 0; c < RC; ++c) {
      const int co = c0 + tc * RC + c;
      if (k <= p.K && co < p.ldw) dst[(size_t)k * p.ldw + co] = acc[a][c];
    }
  }
}

// thread = one element of [K + 1, ldw]: the chunk partials in chunk order
__global__ __launch_bounds__(256) void conv_dw_sum_k(const CbParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x, n = (long)(p.K + 1) * p.ldw;
  if (i >= n) return;
  const float s = ymi_chunk_sum(p.ws, n, p.nchunks, i);
  const long k = i / p.ldw;
  const int co = (int)(i - k * p.ldw);
  if (k < p.K) { if (p.dw) p.dw[i] = s; }
  else if (p.db && co < p.Cout) p.db[co] = s;
}

int reg_tile(int n) { return n <= 16 ? 1 : (n <= 32 ? 2 : 4); }

int validate_conv(const ymi_conv_bwd_desc *d) {
  if (!d) return YMI_ENULL;
  if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride <= 0 || d->pad < 0 ||
      (d->relu != 0 && d->relu != 1))
    return YMI_EARG;
  if (d->Ho < 1 || d->Wo < 1 || d->Ho != (d->H + 2 * d->pad - d->kh) / d->stride + 1 || d->Wo != (d->W + 2 * d->pad - d->kw) / d->stride + 1)
    return YMI_ESHAPE;
  if ((long)d->B * d->H * d->W * d->Cin >= (1L << 40) || (long)d->B * d->Ho * d->Wo * d->Cout >= (1L << 40) ||
      (long)d->kh * d->kw * d->Cin >= (1L << 24) || d->Cout >= (1 << 24))
    return YMI_ESHAPE;
  return YMI_OK;
}

// the decomposition of dw / db for a validated shape
void dw_plan(const ymi_conv_bwd_desc *d, CbParams &p, int &rk, int &rc, int &nkt) {
  p.K = d->kh * d->kw * d->Cin;
  p.ldw = (d->Cout + 3) / 4 * 4;
  p.P = (long)d->B * d->Ho * d->Wo;
  rk = reg_tile(p.K + 1); rc = reg_tile(p.ldw);
  nkt = (p.K + 1 + 16 * rk - 1) / (16 * rk);
  p.nct = (p.ldw + 16 * rc - 1) / (16 * rc);
  const long tiles = (long)nkt * p.nct;
  long want = (p.P + 127) / 128;                     // at least 128 positions per chunk ..
  const long most = 1024 / tiles < 1 ? 1 : 1024 / tiles;   // .. and about 1024 blocks
  want = want > most ? most : want;
  p.chunk = ((p.P + want - 1) / want + PS - 1) / PS * PS;
  p.nchunks = (int)((p.P + p.chunk - 1) / p.chunk);
}

// ---- the pool's backward and the head ---------------------------------------------------------------------------------------------
// thread = (n, c): the first maximum of y[n,:,c] takes d_pool[n,c], the other positions 0
__global__ __launch_bounds__(256) void maxpool_bwd_k(const float *__restrict__ y, const float *__restrict__ d_pool, float *__restrict__ dy,
                                                      int HW, int C, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long n = i / C;
  const int c = (int)(i - n * C);
  const size_t base = (size_t)n * HW * C + c;
  float m = y[base];
  int at = 0;
  for (int q = 1; q < HW; ++q) { const float v = y[base + (size_t)q * C]; if (v > m) { m = v; at = q; } }
  const float g = d_pool[i];
  for (int q = 0; q < HW; ++q) dy[base + (size_t)q * C] = q == at ? g : 0.f;
}

struct HdParams {
  const float *pool, *iou_t;
  const int32_t *label;
  float *loss, *d_pool, *ws;
  int N, C;
  float alpha;
};

// thread = (n, c)
__global__ __launch_bounds__(256) void head_k(const HdParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)p.N * p.C) return;
  const int n = (int)(i / p.C), c = (int)(i - (long)n * p.C);
  const int lab = p.label[n] < 0 ? 0 : (p.label[n] >= p.C ? p.C - 1 : p.label[n]);
  float g = 0.f;
  if (c == lab) {
    const float d = p.pool[i] - p.iou_t[n], a = fabsf(d);
    p.ws[n] = a < 1.f ? 0.5f * d * d : a - 0.5f;     // F.smooth_l1_loss, beta = 1
    g = (a < 1.f ? d : (d > 0.f ? 1.f : -1.f)) * p.alpha;
  }
  if (p.d_pool) p.d_pool[i] = g;
}

__global__ __launch_bounds__(256) void head_sum_k(const HdParams p) {
  const float s = ymi_sum256(p.ws, p.N);
  if (threadIdx.x == 0) p.loss[0] = s * p.alpha;
}

int validate_head(const ymi_maskiou_head_desc *d) {
  if (!d) return YMI_ENULL;
  if (d->N < 1 || d->C < 1 || (long)d->N * d->C >= (1L << 40)) return YMI_EARG;
  return YMI_OK;
}

}  // namespace

// Workspace of ymi_maskiou_input_bwd_f32: [ntiles][N][32] floats
extern "C" int64_t ymi_maskiou_input_ws_bytes(const ymi_maskiou_input_desc *d) {
  const int rc = validate_input(d);
  if (rc) return rc;
  return ymi_ws_part((int64_t)ymi_lincomb_ntiles(d->mh, d->mw) * d->N * 32);
}

extern "C" int ymi_maskiou_input_f32(const ymi_maskiou_input_desc *d, void *stream) {
  int rc = validate_input(d);
  if (rc) return rc;
  rc = validate_input_ptrs(d);
  if (rc) return rc;
  if (!d->gt || !d->gt_idx || !d->x0 || !d->iou_t) return YMI_ENULL;
  return ymi_launch(miou_input_k, dim3(d->N), dim3(256), 0, stream, mi_params(d));
}

extern "C" int ymi_maskiou_input_bwd_f32(const ymi_maskiou_input_desc *d, void *stream) {
  int rc = validate_input(d);
  if (rc) return rc;
  rc = validate_input_ptrs(d);
  if (rc) return rc;
  if (!d->d_x0 || (!d->d_proto && !d->d_coef) || (d->d_coef && !d->ws)) return YMI_ENULL;
  if (((uintptr_t)d->d_proto | (uintptr_t)d->ws) & 15) return YMI_ESHAPE;
  if (d->ws_bytes < (d->d_coef ? ymi_maskiou_input_ws_bytes(d) : 0)) return YMI_ESHAPE;
  MiParams p = mi_params(d);
  const size_t lds = ymi_lincomb_lds<MiTerm>(d->N, CAP_MAX, p.cap);                // <= 22 KB
  rc = ymi_launch(miou_input_bwd_k, dim3(p.ntiles, d->B), dim3(256), lds, stream, p);
  if (!rc && d->d_coef) rc = ymi_launch(miou_dcoef_k, dim3((int)(((long)d->N * 32 + 255) / 256)), dim3(256), 0, stream, p);
  return rc;
}

// Workspace of ymi_conv2d_bwd_nhwc_f32: [nchunks][K + 1][ceil4(Cout)] floats
extern "C" int64_t ymi_conv_bwd_ws_bytes(const ymi_conv_bwd_desc *d) {
  const int rc = validate_conv(d);
  if (rc) return rc;
  CbParams p;
  int rk, rcol, nkt;
  dw_plan(d, p, rk, rcol, nkt);
  if ((long)nkt * p.nct > 65535) return YMI_ESHAPE;   // the tiles of [K + 1, Cout] are the grid's y
  return ymi_ws_part((int64_t)p.nchunks * (p.K + 1) * p.ldw);
}

extern "C" int ymi_conv2d_bwd_nhwc_f32(const ymi_conv_bwd_desc *d, void *stream) {
  int rc = validate_conv(d);
  if (rc) return rc;
  const bool want_w = d->dw || d->db;
  if (!d->dy || (d->relu && !d->y) || (!d->dx && !want_w) || (d->dx && !d->w) || (want_w && (!d->x || !d->ws))) return YMI_ENULL;
  if (((uintptr_t)d->w | (uintptr_t)d->y | (uintptr_t)d->dy | (uintptr_t)d->ws) & 15) return YMI_ESHAPE;
  if (want_w && d->ws_bytes < ymi_conv_bwd_ws_bytes(d)) return YMI_ESHAPE;
  CbParams p;
  p.x = d->x; p.w = d->w; p.y = d->y; p.dy = d->dy; p.dx = d->dx; p.dw = d->dw; p.db = d->db; p.ws = static_cast<float *>(d->ws);
  p.B = d->B; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.Ho = d->Ho; p.Wo = d->Wo; p.Cout = d->Cout;
  p.kh = d->kh; p.kw = d->kw; p.stride = d->stride; p.pad = d->pad; p.relu = d->relu;
  int rk, rcol, nkt;
  dw_plan(d, p, rk, rcol, nkt);
  if (want_w && (long)nkt * p.nct > 65535) return YMI_ESHAPE;
  if (d->dx) {
    const int ct = d->Cin % 4 == 0 ? 4 : 1;
    p.total = (long)d->B * d->H * d->W * (d->Cin / ct);
    const dim3 grid((unsigned)((p.total + 255) / 256));
    rc = ct == 4 ? ymi_launch(conv_dx_k<4>, grid, dim3(256), 0, stream, p) : ymi_launch(conv_dx_k<1>, grid, dim3(256), 0, stream, p);
    if (rc) return rc;
  }
  if (want_w) {
    const dim3 grid(p.nchunks, nkt * p.nct);
    void (*k)(CbParams) = nullptr;
#define YMI_DW(A, C) if (rk == A && rcol == C) k = conv_dw_k<A, C>;
    YMI_DW(1, 1) YMI_DW(1, 2) YMI_DW(1, 4) YMI_DW(2, 1) YMI_DW(2, 2) YMI_DW(2, 4) YMI_DW(4, 1) YMI_DW(4, 2) YMI_DW(4, 4)
#undef YMI_DW
    rc = ymi_launch(k, grid, dim3(256), 0, stream, p);
    if (!rc) rc = ymi_launch(conv_dw_sum_k, dim3((unsigned)(((long)(p.K + 1) * p.ldw + 255) / 256)), dim3(256), 0, stream, p);
  }
  return rc;
}

extern "C" int ymi_global_maxpool_bwd_nhwc_f32(const float *y, const float *d_pool, float *dy, int B, int HW, int C, void *stream) {
  if (!y || !d_pool || !dy) return YMI_ENULL;
  if (B <= 0 || HW <= 0 || C <= 0) return YMI_EARG;
  const long total = (long)B * C;
  hipLaunchKernelGGL(maxpool_bwd_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, d_pool, dy, HW, C, total);
  return ymi_launch_status();
}

// Workspace of ymi_maskiou_head_f32: [N] floats
extern "C" int64_t ymi_maskiou_head_ws_bytes(const ymi_maskiou_head_desc *d) {
  const int rc = validate_head(d);
  if (rc) return rc;
  return ymi_ws_part(d->N);
}

extern "C" int ymi_maskiou_head_f32(const ymi_maskiou_head_desc *d, void *stream) {
  const int rc = validate_head(d);
  if (rc) return rc;
  if (!d->pool || !d->iou_t || !d->label || !d->loss || !d->ws) return YMI_ENULL;
  if (d->ws_bytes < ymi_maskiou_head_ws_bytes(d)) return YMI_ESHAPE;
  HdParams p;
  p.pool = d->pool; p.iou_t = d->iou_t; p.label = d->label; p.loss = d->loss; p.d_pool = d->d_pool; p.ws = static_cast<float *>(d->ws);
  p.N = d->N; p.C = d->C; p.alpha = d->alpha;
  int rl = ymi_launch(head_k, dim3((unsigned)(((long)d->N * d->C + 255) / 256)), dim3(256), 0, stream, p);
  if (!rl) rl = ymi_launch(head_sum_k, dim3(1), dim3(256), 0, stream, p);
  return rl;
}
