// The data gradient of a STRIDE-2 convolution (3x3 / pad 1 and 1x1 / pad 0), NHWC fp32, for the backbone's stage entries (each stage's
// first conv2 and the projection shortcuts, backbone.py:28-29, 94-99), whose maps reach 138 x 138: the zero-insert route of
// train_ops._data_grad (zero_insert, which conv2d_down keeps for the FPN's small maps) spends four times the useful FLOPs there.
//
//   ymi_conv_dgrad_s2_nhwc_f32   dx[n,y,x,ci] = sum over the taps (ky, kx) that EXIST for this pixel, sum_co g[n,oy,ox,co] w[co,ci,ky,kx]
//                                with oy = (y + pad - ky) / 2 where that division is exact and 0 <= oy < Ho (the same in x).
//
// Only existing taps are computed.  The input pixels fall into four parity phases (y & 1, x & 1).  At 3x3 an even y has the one row tap
// ky = 1 (oy = y / 2), an odd y the two row taps ky = 0 (oy = (y + 1) / 2, outside g for the last odd row of an even H: masked) and
// ky = 2 (oy = (y - 1) / 2); the phases have 1, 2, 2 and 4 taps, 9 tap-products per 2 x 2 pixels.  At 1x1 the even / even phase has one
// tap and every other pixel is written as +0.0.
//
// A block owns 256 pixels of ONE phase (in (n, y, x) order within the phase) and 64 input channels; each of its four waves 64 pixels
// (two column tiles of 32) and the block's channels (two row tiles of 32), four accumulators of v_mfma_f32_32x32x2_f32 (fp32 in, fp32
// accumulate) with Cout as the instruction's k index: A = the filter (row = ci), B = g (column = pixel).  Both operands come as
// 16-byte loads: lane (i, h) reads g[pixel i][8 q + 4 h .. + 3] and the packed filter [tap][Cout / 4][Cin][4] at (2 q + h, ci i), one
// step q (8 output channels = 4 instructions per accumulator) ahead of the MFMAs that use them.  A masked tap or a pixel past the phase
// reads element 0 and is replaced by 0.
//
// SUMMATION ORDER (part of the contract; a function of the shape only): every element of dx starts from +0.0 and adds its taps with ky
// ascending, within ky kx ascending; within a tap q = 0 .. Cout / 8 - 1 ascending, within q the instructions e = 0 .. 3, and instruction
// (q, e) adds the two products of co = 8 q + e and co = 8 q + 4 + e (the instruction's k = 0, 1).  A masked tap adds products with a
// zero factor.  Every element of dx is written exactly once, by one lane; no atomics; the same inputs give the same bits.
#include "loss_common.h"
#include "../../include/yolact_amd.h"

namespace {

struct DgParams {
  const float *g, *w;
  float *dx;
  int B, H, W, Cin, Cout, ldg, Ho, Wo;
  int blk_end[4];                                      // blocks of the phases (1,1), (1,0), (0,1), (0,0), cumulative
};

// K3: 3x3 / pad 1 (else 1x1 / pad 0)
template <bool K3> __global__ __launch_bounds__(256, 2) void dgrad_s2_k(const DgParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ln = lane & 31, h = lane >> 5;
  int ph = 0;
  while (ph < 3 && (int)blockIdx.x >= p.blk_end[ph]) ++ph;
  const int py = ph < 2 ? 1 : 0, px = (ph & 1) ? 0 : 1;
  const int blk0 = ph ? p.blk_end[ph - 1] : 0;
  const int Hp = (p.H - py + 1) / 2, Wp = (p.W - px + 1) / 2;          // the pixels of this parity along each axis
  const int Pph = p.B * Hp * Wp;
  const int pbase = ((int)blockIdx.x - blk0) * 256 + wave * 64;
  if (pbase >= Pph) return;                            // (no barrier below)
  const int cb = (int)blockIdx.y * 64;
  const int nci = cb + 32 < p.Cin ? 2 : 1;             // the wave's row tiles that hold real channels (Cin % 32 == 0)

  // this lane's two pixels
  bool valid[2];
  int pa[2], pb[2], pn[2];
  unsigned doff[2];                                    // byte offset of the pixel in dx (validate: below 2^31)
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int pi = pbase + m * 32 + ln;
    valid[m] = pi < Pph;
    const int q = valid[m] ? pi : 0;
    pn[m] = q / (Hp * Wp);
    const int r = q - pn[m] * (Hp * Wp);
    pa[m] = r / Wp;
    pb[m] = r - pa[m] * Wp;
    doff[m] = 4u * (unsigned)(((pn[m] * p.H + 2 * pa[m] + py) * p.W + 2 * pb[m] + px) * p.Cin + cb);
  }

  const int nty = K3 ? 1 + py : 1, ntx = K3 ? 1 + px : 1;
  const int ntap = K3 ? nty * ntx : (ph == 3 ? 1 : 0);
  const int nq = p.Cout / 8, C4 = p.Cout / 4;

  f32x16 acc[2][2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][m][r] = 0.f;

  const char *gb = reinterpret_cast<const char *>(p.g), *wb = reinterpret_cast<const char *>(p.w);
  // the state of the NEXT step to load: tap (it_tap), step (it_q), the tap's offsets and masks
  int it_tap = 0, it_q = 0;
  unsigned goff[2], woff = 0;
  bool gm[2] = {false, false};
  auto setup = [&](int tapi) {
    const int ty = tapi / ntx, tx = tapi - ty * ntx;
    // 3x3: an odd coordinate has the taps k = 0 (output index + 1) and k = 2 (output index + 0), an even one k = 1; 1x1: k = 0
    const int ky = K3 ? (py ? 2 * ty : 1) : 0, kx = K3 ? (px ? 2 * tx : 1) : 0;
    const int dy = (K3 && py) ? 1 - ty : 0, dxx = (K3 && px) ? 1 - tx : 0;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int oy = pa[m] + dy, ox = pb[m] + dxx;
      gm[m] = valid[m] && oy < p.Ho && ox < p.Wo;
      goff[m] = gm[m] ? 4u * (unsigned)(((pn[m] * p.Ho + oy) * p.Wo + ox) * p.ldg) : 0u;
    }
    woff = 16u * (unsigned)(((ky * (K3 ? 3 : 1) + kx) * C4 + h) * p.Cin + cb + ln);
  };
  struct Op { f32x4 a[2], b[2]; bool m[2]; };
  auto issue = [&](Op &o) {
    const unsigned wq = woff + 32u * (unsigned)(it_q * p.Cin);        // group 2 q + h of four output channels
    const unsigned gq = 32u * (unsigned)it_q + 16u * (unsigned)h;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (c < nci) o.a[c] = *reinterpret_cast<const f32x4 *>(wb + (wq + 512u * c));
      else o.a[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      o.b[m] = *reinterpret_cast<const f32x4 *>(gb + (goff[m] + gq));
      o.m[m] = gm[m];
    }
    if (++it_q == nq) {
      it_q = 0;
      if (++it_tap < ntap) setup(it_tap);
    }
  };
  auto consume = [&](const Op &o) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const float b = o.m[m] ? o.b[m][e] : 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c)
          if (c < nci) acc[c][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.a[c][e], b, acc[c][m], 0, 0, 0);
      }
    }
  };
  const int T = ntap * nq;                             // even: Cout % 32 == 0
  if (T > 0) {
    Op O0, O1;
    setup(0);
    issue(O0);
    for (int it = 0; it < T; it += 2) {
      issue(O1);
      consume(O0);
      if (it + 2 < T) issue(O0);
      consume(O1);
    }
  }

  // lane (i, h) holds of pixel i the channels (r & 3) + 8 (r >> 2) + 4 h of each row tile (grad_common.h ymi_acc_row): four 16-byte stores
  char *db = reinterpret_cast<char *>(p.dx);
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    if (!valid[m]) continue;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (c >= nci) continue;
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const f32x4 v = {acc[c][m][4 * rg], acc[c][m][4 * rg + 1], acc[c][m][4 * rg + 2], acc[c][m][4 * rg + 3]};
        *reinterpret_cast<f32x4 *>(db + (doff[m] + 4u * (unsigned)(c * 32 + 8 * rg + 4 * h))) = v;
      }
    }
  }
#endif
}

inline int dgrad_out(int size, int k, int pad) { return (size + 2 * pad - k) / 2 + 1; }

int validate_dgrad(const ymi_conv_dgrad_desc *d) {
  if (!d) return YMI_ENULL;
  if (d->B < 1 || d->H < 1 || d->W < 1 || d->Cin < 1 || d->Cout < 1 || d->ldg < 1) return YMI_EARG;
  if (!((d->kh == 3 && d->kw == 3 && d->pad == 1) || (d->kh == 1 && d->kw == 1 && d->pad == 0)) || d->stride != 2) return YMI_EARG;
  if (d->Cin % 32 != 0 || d->Cout % 32 != 0 || d->ldg < d->Cout || d->ldg % 4 != 0) return YMI_ESHAPE;
  const long Ho = dgrad_out(d->H, d->kh, d->pad), Wo = dgrad_out(d->W, d->kw, d->pad);
  if ((long)d->B * d->H * d->W * d->Cin >= (1L << 29) || (long)d->B * Ho * Wo * d->ldg >= (1L << 29) ||
      (long)d->kh * d->kw * d->Cin * d->Cout >= (1L << 29)) return YMI_ESHAPE;
  if (!d->g || !d->w || !d->dx) return YMI_ENULL;
  if (((uintptr_t)d->g | (uintptr_t)d->w | (uintptr_t)d->dx) & 15) return YMI_ESHAPE;
  return YMI_OK;
}

}  // namespace

extern "C" int ymi_conv_dgrad_s2_nhwc_f32(const ymi_conv_dgrad_desc *d, void *stream) {
  const int rc = validate_dgrad(d);
  if (rc) return rc;
  DgParams p;
  p.g = d->g; p.w = d->w; p.dx = d->dx;
  p.B = d->B; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.Cout = d->Cout; p.ldg = d->ldg;
  p.Ho = dgrad_out(d->H, d->kh, d->pad); p.Wo = dgrad_out(d->W, d->kw, d->pad);
  long at = 0;
  for (int ph = 0; ph < 4; ++ph) {                     // the four-tap phase first: the longest blocks start first
    const int py = ph < 2 ? 1 : 0, px = (ph & 1) ? 0 : 1;
    const long n = (long)d->B * ((d->H - py + 1) / 2) * ((d->W - px + 1) / 2);
    at += (n + 255) / 256;
    p.blk_end[ph] = (int)at;
  }
  const dim3 grid((unsigned)at, (unsigned)((d->Cin + 63) / 64));
  return d->kh == 3 ? ymi_launch(dgrad_s2_k<true>, grid, dim3(256), 0, stream, p)
                    : ymi_launch(dgrad_s2_k<false>, grid, dim3(256), 0, stream, p);
}
