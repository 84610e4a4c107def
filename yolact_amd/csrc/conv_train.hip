// The backward of the train-mode heads and protonet (yolact.py:133-212, 580-647; utils/functions.py:163-213): stride-1 convolutions
// (3x3 / pad 1, 1x1 / pad 0), ReLU, tanh and the x2 bilinear upsample, NHWC fp32, without floating-point atomics (the same inputs
// give the same bits).  The data gradient of a convolution is a convolution again and runs on ymi_conv2d_nhwc_f32; what is new here:
//
//   ymi_act_bwd_f32             g[pos,c] = dy[pos,c] * act'(y[pos,c]) from the layer's OUTPUT y (ReLU: y > 0, tanh: 1 - y^2), written
//                               with the channel stride the consumers want; the padding channels get exact zeros.
//   ymi_conv_wgrad_nhwc_f32     dw[k,co] = sum_pos im2col(x)[pos,k] g[pos,co], db[co] = sum_pos g[pos,co] in the structure of
//                               grad_common.h (positions = the matrix instruction's k index, chunk partials, an ordered sum).  A
//                               block owns one (tap, 32 input channels), a chunk of positions and NT * 128 output channels (each wave
//                               NT column tiles of 32); the tap only shifts the address of x, a shifted pixel outside the image
//                               contributes 0.  Every instruction needs one 4-byte load per lane and operand, so the loads of 32
//                               positions are issued as a group, one group ahead of the MFMAs that use them (two waves per SIMD for
//                               NT <= 2, one for NT = 4: 198 / 250 / 357 registers, no spills).  db falls out of the g fragments of
//                               the blocks of (tap 0, chunk 0 of the channels).
//   ymi_bilinear_bwd_nhwc_f32   the backward of ymi_bilinear_nhwc_f32 for Ho = 2 Hi, Wo = 2 Wi as a gather: an input pixel (iy, ix)
//                               walks the output rows 2 iy - 2 .. 2 iy + 2 and columns 2 ix - 2 .. 2 ix + 2 in order, asks
//                               upsample_math.h which of them read it and with what weight, and sums.
//
// The backward of the train-mode FPN (yolact.py:311-360) adds two things: a stride (1 or 2) in the weight gradient, as a template
// parameter of wgrad_k (the positions stay those of g, the stride only changes which pixel of x a tap reads), and
//   ymi_bilinear_size_bwd_nhwc_f32   the backward of the size-form interpolation for any Ho >= Hi, Wo >= Wi (the pyramid of a 550 x 550
//                               image is 69 -> 35 -> 18: neither step is x2), the same gather with the candidate outputs found by
//                               inverting the coordinate map.
#include "wgrad_plan.h"
#include "upsample_math.h"

namespace {

// ---- activation backward ------------------------------------------------------------------------------------------------------------
struct AbParams {
  const float *y, *dy;
  float *g;
  long total;
  int C, cpad, ldy, lddy, ldg, act;
};

// thread = (position, channel of [0, cpad))
__global__ __launch_bounds__(256) void act_bwd_k(const AbParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const long pos = i / p.cpad;
  const int c = (int)(i - pos * p.cpad);
  float v = 0.f;
  if (c < p.C) {
    v = p.dy[(size_t)pos * p.lddy + c];
    if (p.act == YMI_ACT_RELU) {
      v = p.y[(size_t)pos * p.ldy + c] > 0.f ? v : 0.f;
    } else if (p.act == YMI_ACT_TANH) {
      const float yv = p.y[(size_t)pos * p.ldy + c];
      v = v * (1.f - yv * yv);
    }
  }
  p.g[(size_t)pos * p.ldg + c] = v;
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------------
struct WgParams {
  const float *x, *g;
  float *dw, *db, *ws_w, *ws_b;
  int H, W, Cin, Cout, ldg, kw, pad, ncc, K, nchunks, want_w, want_b;
  long P, per;
  int Ho, Wo;                                          // the map of g (stride 2; H, W at stride 1)
};

// NT: 32-column output-channel tiles per wave (a block covers NT * 128 output channels, gridDim.z such groups)
// S: the convolution's stride, 1 or 2.  A template parameter, so that the stride-1 instantiation carries nothing of stride 2: the
// positions are those of g, [B, Ho, Wo]; at stride 2 tap (ky, kx) of position (n, oy, ox) reads x at (2 oy + ky - pad, 2 ox + kx - pad).
template <int NT, int S> __global__ __launch_bounds__(256, NT == 4 ? 1 : 2) void wgrad_k(const WgParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ln = lane & 31, kk = lane >> 5;
  const int tap = (int)blockIdx.x / p.ncc, c0 = ((int)blockIdx.x % p.ncc) * 32;
  const int ky = tap / p.kw, kx = tap - ky * p.kw;
  const int sy = ky - p.pad, sx = kx - p.pad;          // the tap's shift of the input pixel
  const int ob = blockIdx.z * (NT * 128);
  const long pos0 = (long)blockIdx.y * p.per;
  const long pos1 = pos0 + p.per < p.P ? pos0 + p.per : p.P;
  const bool do_w = p.want_w != 0;
  const bool do_bias = p.want_b != 0 && blockIdx.x == 0;

  // the wave's column tiles that hold a real output channel are a prefix of its NT tiles
  int nact = 0;
#pragma unroll
  for (int j = 0; j < NT; ++j) nact += (ob + (wave + 4 * j) * 32 < p.Cout) ? 1 : 0;
  if (nact == 0) return;                               // (no barrier below)

  f32x16 acc[NT];
  float bs[NT];
  unsigned gc[NT];                                     // byte offset in g of this lane's channel of tile j (channel 0 where the tile has none)
  bool col[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    bs[j] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    const int o = ob + (wave + 4 * j) * 32 + ln;
    col[j] = o < p.Cout;
    gc[j] = 4u * (unsigned)(col[j] ? o : 0);
  }

  // this lane's positions: pos0 + kk, + 2, + 4, ..; their pixel coordinates are carried along (grad_common.h: why not ymi_pos_walk)
  long pos = pos0 + kk;
  const int PW = S == 1 ? p.W : p.Wo, PH = S == 1 ? p.H : p.Ho;   // the map the positions run over
  int ox = (int)(pos % PW), oy = (int)((pos / PW) % PH);
  int n = S == 1 ? 0 : (int)(pos / ((long)PW * PH));   // stride 2 only: the image, for the address of x
  // byte offsets fit 32 bits (validate_wgrad): a uniform base plus one register per load
  const int xlane = 4 * (c0 + ln), shift = 4 * ((sy * p.W + sx) * p.Cin);
  const char *xb = reinterpret_cast<const char *>(p.x), *gb = reinterpret_cast<const char *>(p.g);
  const unsigned xstep = 4u * (unsigned)p.Cin, gstep = 4u * (unsigned)p.ldg;

  // One group = 32 positions = 16 instructions.  All loads of a group are issued before its first MFMA, and the next group's are
  // issued before this group's MFMAs, so that the memory latency hides under the matrix pipe.  The loads are unconditional: a
  // position past the chunk or a shifted pixel outside the image reads element 0 instead and is zeroed by its mask bit afterwards.
  struct Grp { float a[16]; float b[NT][16]; unsigned am, lm; };
  auto issue = [&](Grp &G) {
    G.am = 0u; G.lm = 0u;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const bool live = pos < pos1;
      const bool inside = live && (unsigned)(S * oy + sy) < (unsigned)p.H && (unsigned)(S * ox + sx) < (unsigned)p.W;
      G.lm |= (live ? 1u : 0u) << s;
      G.am |= (inside ? 1u : 0u) << s;
      unsigned xo;
      if constexpr (S == 1) {
        xo = (inside ? (unsigned)((int)((unsigned)pos * xstep) + shift) : 0u) + (unsigned)xlane;
      } else {
        xo = (inside ? (unsigned)((n * p.H + S * oy + sy) * p.W + S * ox + sx) * xstep : 0u) + (unsigned)xlane;
      }
      G.a[s] = do_w ? *reinterpret_cast<const float *>(xb + xo) : 0.f;
      const unsigned gi = live ? (unsigned)pos * gstep : 0u;
#pragma unroll
      for (int j = 0; j < NT; ++j) G.b[j][s] = j < nact ? *reinterpret_cast<const float *>(gb + (gi + gc[j])) : 0.f;
      pos += 2; ox += 2;
      if (ox >= PW) { ox -= PW; ++oy; }                 // twice: W may be 1
      if (ox >= PW) { ox -= PW; ++oy; }
      if constexpr (S == 1) {
        if (oy >= PH) oy -= PH;
        if (oy >= PH) oy -= PH;
      } else {
        if (oy >= PH) { oy -= PH; ++n; }
        if (oy >= PH) { oy -= PH; ++n; }
      }
    }
  };
  auto consume = [&](const Grp &G) {
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float a = (G.am >> s & 1u) ? G.a[s] : 0.f;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        if (j < nact) {
          const float b = ((G.lm >> s & 1u) && col[j]) ? G.b[j][s] : 0.f;
          bs[j] += b;
          if (do_w) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[j], 0, 0, 0);
        }
      }
    }
  };
  Grp G0, G1;
  issue(G0);
  for (long m0 = pos0; m0 < pos1; m0 += 64) {
    issue(G1);                                         // (past the chunk: every mask bit is 0)
    consume(G0);
    issue(G0);
    consume(G1);
  }

  if (do_w) {
    float *dst = p.ws_w + (size_t)blockIdx.y * p.K * p.Cout + ((size_t)tap * p.Cin + c0) * p.Cout;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int o = ob + (wave + 4 * j) * 32 + ln;
      if (j < nact && o < p.Cout) {
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(size_t)ymi_acc_row(r, kk) * p.Cout + o] = acc[j][r];
      }
    }
  }
  if (do_bias) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const float v = bs[j] + __shfl_xor(bs[j], 32);   // even positions + odd positions
      const int o = ob + (wave + 4 * j) * 32 + ln;
      if (j < nact && kk == 0 && o < p.Cout) p.ws_b[(size_t)blockIdx.y * p.Cout + o] = v;
    }
  }
#endif
}

// thread = one element of dw [K, Cout], then of db [Cout]
__global__ __launch_bounds__(256) void wgrad_sum_k(const WgParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x, nw = (long)p.K * p.Cout;
  if (i < nw) {
    if (!p.want_w) return;
    p.dw[i] = ymi_chunk_sum(p.ws_w, nw, p.nchunks, i);
  } else if (i < nw + p.Cout) {
    if (!p.want_b) return;
    const int o = (int)(i - nw);
    p.db[o] = ymi_chunk_sum(p.ws_b, p.Cout, p.nchunks, o);
  }
}

// ---- x2 bilinear upsample backward ----------------------------------------------------------------------------------------------------
struct UbParams {
  const float *dy, *y;
  float *dx;
  int Hi, Wi, C4, Ho, Wo, relu;
  long total;
};

// the weight with which output index o reads input index i along one axis (0 when it does not)
__device__ __forceinline__ float up_weight(int o, int i, int in_size) {
  int i0, i1; float l1;
  up_coord(o, 0.5f, in_size, i0, i1, l1);
  return (i0 == i ? 1.f - l1 : 0.f) + (i1 == i ? l1 : 0.f);
}

// thread = (input pixel, 4 channels)
__global__ __launch_bounds__(256) void bilinear_bwd_k(const UbParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const int c4 = (int)(i % p.C4);
  long r = i / p.C4;
  const int ix = (int)(r % p.Wi); r /= p.Wi;
  const int iy = (int)(r % p.Hi);
  const long b = r / p.Hi;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int oy = 2 * iy - 2; oy <= 2 * iy + 2; ++oy) {
    if (oy < 0 || oy >= p.Ho) continue;
    const float wy = up_weight(oy, iy, p.Hi);
    if (wy == 0.f) continue;
    for (int ox = 2 * ix - 2; ox <= 2 * ix + 2; ++ox) {
      if (ox < 0 || ox >= p.Wo) continue;
      const float wx = up_weight(ox, ix, p.Wi);
      if (wx == 0.f) continue;
      const size_t o = (((size_t)b * p.Ho + oy) * p.Wo + ox) * p.C4 * 4 + (size_t)c4 * 4;
      f32x4 d = *reinterpret_cast<const f32x4 *>(p.dy + o);
      if (p.relu) {
        const f32x4 yv = *reinterpret_cast<const f32x4 *>(p.y + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = yv[e] > 0.f ? d[e] : 0.f;
      }
      const float w = wy * wx;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += w * d[e];
    }
  }
  *reinterpret_cast<f32x4 *>(p.dx + (size_t)i * 4) = acc;
}

// ---- size-form bilinear backward (any Ho >= Hi, Wo >= Wi) ------------------------------------------------------------------------------
struct UsParams {
  const float *dy;
  float *dx;
  int Hi, Wi, C4, Ho, Wo;
  float sh, sw;
  long total;
};

__device__ __forceinline__ float up_weight_s(int o, float scale, int i, int in_size) {
  int i0, i1; float l1;
  up_coord(o, scale, in_size, i0, i1, l1);
  return (i0 == i ? 1.f - l1 : 0.f) + (i1 == i ? l1 : 0.f);   // the clamped last row: i1 == i0, both terms count
}

// The output indices that can read input index i: i0 == i or i1 == i needs the source coordinate (o + 1/2) in / out - 1/2 inside
// (i - 1, i + 1), that is o inside ((2 i - 1) out / (2 in) - 1/2, (2 i + 3) out / (2 in) - 1/2).  Integer bounds around that, one more
// index each side for the fp32 rounding of the forward's coordinate, clipped; up_coord decides within.
__device__ __forceinline__ void up_candidates(int i, int in_size, int out_size, int &lo, int &hi) {
  const long a = (2L * i - 1) * out_size, b = (2L * i + 3) * out_size, d2 = 2L * in_size;
  long l = (a > 0 ? a / d2 : 0) - 2, h = (b + d2 - 1) / d2 + 1;
  lo = (int)(l < 0 ? 0 : l);
  hi = (int)(h > out_size - 1 ? out_size - 1 : h);
}

// thread = (input pixel, 4 channels); output rows ascending, within a row columns ascending
__global__ __launch_bounds__(256) void bilinear_size_bwd_k(const UsParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const int c4 = (int)(i % p.C4);
  long r = i / p.C4;
  const int ix = (int)(r % p.Wi); r /= p.Wi;
  const int iy = (int)(r % p.Hi);
  const long b = r / p.Hi;
  int oy0, oy1, ox0, ox1;
  up_candidates(iy, p.Hi, p.Ho, oy0, oy1);
  up_candidates(ix, p.Wi, p.Wo, ox0, ox1);
  // -0.0 is the identity of the addition (+0.0 would turn a lone -0.0 into +0.0); for Ho >= Hi, Wo >= Wi every input pixel is read
  // with a non-zero weight by some output pixel, so the start value never reaches dx
  f32x4 acc = {-0.f, -0.f, -0.f, -0.f};
  for (int oy = oy0; oy <= oy1; ++oy) {
    const float wy = up_weight_s(oy, p.sh, iy, p.Hi);
    if (wy == 0.f) continue;
    for (int ox = ox0; ox <= ox1; ++ox) {
      const float wx = up_weight_s(ox, p.sw, ix, p.Wi);
      if (wx == 0.f) continue;
      const f32x4 d = *reinterpret_cast<const f32x4 *>(p.dy + ((((size_t)b * p.Ho + oy) * p.Wo + ox) * p.C4 + c4) * 4);
      const float w = wy * wx;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += w * d[e];
    }
  }
  *reinterpret_cast<f32x4 *>(p.dx + (size_t)i * 4) = acc;
}

}  // namespace

extern "C" int ymi_act_bwd_f32(const float *y, const float *dy, float *g, long npos, int C, int cpad, int ldy, int lddy, int ldg, int act,
                               void *stream) {
  if (!dy || !g) return YMI_ENULL;
  if (act != YMI_ACT_NONE && act != YMI_ACT_RELU && act != YMI_ACT_TANH) return YMI_EARG;
  if (act != YMI_ACT_NONE && !y) return YMI_ENULL;
  if (npos < 1 || C < 1) return YMI_EARG;
  if (cpad < C || ldg < cpad || lddy < C || (act != YMI_ACT_NONE && ldy < C)) return YMI_ESHAPE;
  if (npos * (long)ldg >= (1L << 40) || npos * (long)cpad >= (1L << 39)) return YMI_ESHAPE;
  AbParams p;
  p.y = y; p.dy = dy; p.g = g; p.total = npos * cpad; p.C = C; p.cpad = cpad; p.ldy = ldy; p.lddy = lddy; p.ldg = ldg; p.act = act;
  return ymi_launch(act_bwd_k, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, stream, p);
}

// Workspace of ymi_conv_wgrad_nhwc_f32: [nchunks][kh*kw*Cin][Cout] floats, then [nchunks][Cout] floats
extern "C" int64_t ymi_conv_wgrad_ws_bytes(const ymi_conv_wgrad_desc *d) {
  const int rc = validate_wgrad(d);
  if (rc) return rc;
  const WgPlan w = wgrad_plan(d);
  if (w.gz > 65535) return YMI_ESHAPE;
  const int64_t K = (int64_t)d->kh * d->kw * d->Cin;
  return ymi_ws_part((int64_t)w.nchunks * K * d->Cout) + ymi_ws_part((int64_t)w.nchunks * d->Cout);
}

extern "C" int ymi_conv_wgrad_nhwc_f32(const ymi_conv_wgrad_desc *d, void *stream) {
  const int rc = validate_wgrad(d);
  if (rc) return rc;
  if (!d->g || (!d->dw && !d->db) || (d->dw && !d->x) || !d->ws) return YMI_ENULL;
  if ((uintptr_t)d->ws & 15) return YMI_ESHAPE;
  const WgPlan w = wgrad_plan(d);
  if (w.gz > 65535 || d->ws_bytes < ymi_conv_wgrad_ws_bytes(d)) return YMI_ESHAPE;
  WgParams p;
  p.x = d->x; p.g = d->g; p.dw = d->dw; p.db = d->db;
  p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.Cout = d->Cout; p.ldg = d->ldg; p.kw = d->kw; p.pad = d->pad;
  p.ncc = d->Cin / 32; p.K = d->kh * d->kw * d->Cin; p.nchunks = w.nchunks; p.want_w = d->dw != nullptr; p.want_b = d->db != nullptr;
  p.P = wgrad_positions(d); p.per = w.per; p.Ho = wgrad_out(d, d->H, d->kh); p.Wo = wgrad_out(d, d->W, d->kw);
  p.ws_w = static_cast<float *>(d->ws);
  p.ws_b = reinterpret_cast<float *>(static_cast<char *>(d->ws) + ymi_ws_part((int64_t)w.nchunks * p.K * d->Cout));
  const dim3 grid(d->dw ? w.gx : 1, w.nchunks, w.gz);     // bias alone: the blocks of tap 0, channels 0 .. 31
  void (*const kernels[2][3])(WgParams) = {{wgrad_k<1, 1>, wgrad_k<2, 1>, wgrad_k<4, 1>}, {wgrad_k<1, 2>, wgrad_k<2, 2>, wgrad_k<4, 2>}};
  int rl = ymi_launch(kernels[d->stride == 2][w.nt >> 1], grid, dim3(256), 0, stream, p);      // nt = 1, 2, 4
  if (!rl) rl = ymi_launch(wgrad_sum_k, dim3((unsigned)(((long)p.K * d->Cout + d->Cout + 255) / 256)), dim3(256), 0, stream, p);
  return rl;
}

extern "C" int ymi_bilinear_bwd_nhwc_f32(const float *dy, const float *y, float *dx, int B, int Hi, int Wi, int C, int Ho, int Wo, int relu,
                                         void *stream) {
  if (!dy || !dx || (relu && !y)) return YMI_ENULL;
  if (B < 1 || Hi < 1 || Wi < 1 || C < 1 || (relu != 0 && relu != 1)) return YMI_EARG;
  if (Ho != 2 * Hi || Wo != 2 * Wi || C % 4 != 0) return YMI_ESHAPE;
  if ((long)B * Ho * Wo * C >= (1L << 40)) return YMI_ESHAPE;
  if (((uintptr_t)dy | (uintptr_t)y | (uintptr_t)dx) & 15) return YMI_ESHAPE;
  UbParams p;
  p.dy = dy; p.y = y; p.dx = dx; p.Hi = Hi; p.Wi = Wi; p.C4 = C / 4; p.Ho = Ho; p.Wo = Wo; p.relu = relu;
  p.total = (long)B * Hi * Wi * (C / 4);
  return ymi_launch(bilinear_bwd_k, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, stream, p);
}

extern "C" int ymi_bilinear_size_bwd_nhwc_f32(const float *dy, float *dx, int B, int Hi, int Wi, int C, int Ho, int Wo, void *stream) {
  if (!dy || !dx) return YMI_ENULL;
  if (B < 1 || Hi < 1 || Wi < 1 || C < 1 || Ho < 1 || Wo < 1) return YMI_EARG;
  if (Ho < Hi || Wo < Wi || C % 4 != 0) return YMI_ESHAPE;
  if ((double)B * Ho * Wo * C >= 0x1p40) return YMI_ESHAPE;
  if (((uintptr_t)dy | (uintptr_t)dx) & 15) return YMI_ESHAPE;
  UsParams p;
  p.dy = dy; p.dx = dx; p.Hi = Hi; p.Wi = Wi; p.C4 = C / 4; p.Ho = Ho; p.Wo = Wo;
  p.sh = (float)Hi / (float)Ho; p.sw = (float)Wi / (float)Wo;       // as ymi_bilinear_nhwc_f32 derives them from the sizes
  p.total = (long)B * Hi * Wi * (C / 4);
  return ymi_launch(bilinear_size_bwd_k, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, stream, p);
}
