// The weight gradient of the train-mode DarkNet53 pre-convolution (backbone.py:268: 3x3 / stride 1 / pad 1 on 3 channels, no bias),
// NHWC fp32, without atomics (the same inputs give the same bits).  The forward convolution runs on ymi_conv2d_nhwc_f32 (the Cin-4
// loader), BatchNorm + LeakyReLU(0.1) on csrc/bn_train.hip (ymi_bn_leaky_*); every other DarkNet convolution has a multiple of 32
// input channels and runs on conv_train.hip / conv_dgrad.hip.  What is new here:
//
//   ymi_preconv_wgrad_nhwc_f32  dw[k,co] = sum_pos x[n, oy + ky - 1, ox + kx - 1, ci] g[pos,co], k = (ky*3 + kx)*3 + ci (27 rows), in the
//                               structure of grad_common.h (positions = the matrix instruction's k index, chunk partials, an ordered
//                               sum).  x is the NHWC-4 image the forward reads.  As in stem_wgrad_k every A-operand lane loads its own
//                               element, so the 27 rows (ky, kx, ci) are rows 0 .. 26 of ONE 32-row tile (rows 27 .. 31 are masked
//                               and never stored): one instruction per two positions and 32 output channels, no split over ky.  The
//                               B operand is 32 consecutive channels of g.  A block is ONE wave that owns a chunk of positions and 32
//                               output channels: 16 accumulator registers.  A tap outside the image, a row past 26 and a position
//                               past the chunk are masked to 0 by a select, never by a product; channel 3 of x is never addressed.
//                               So the padding channel may hold anything, NaN included.
//
// THE CHUNKS follow ymi_chunk_plan with a target of 2048 blocks (the stem's is 512): a block is one wave here, not four, and the real
// shape (8 x 550 x 550, Cout = 32) has a single channel group, so 2048 chunks are what puts eight waves on each of the 256 CUs.
#include "grad_common.h"
#include "../../include/yolact_amd.h"

namespace {

struct PwParams {
  const float *x, *g;
  float *dw, *ws;
  int H, W, Cout, ldg, nchunks;
  long P, per;
};

constexpr int PW_K = 27;                               // 3 * 3 * 3 rows of dw
constexpr int PW_G = 8;                                // instructions per load group (16 positions)

__global__ __launch_bounds__(64) void preconv_wgrad_k(const PwParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int lane = threadIdx.x, ln = lane & 31, kk = lane >> 5;
  const int ob = blockIdx.z * 32;
  const long pos0 = (long)blockIdx.y * p.per;
  const long pos1 = pos0 + p.per < p.P ? pos0 + p.per : p.P;
  const bool row_used = ln < PW_K;
  const int tap = ln / 3, ci = ln - 3 * tap;           // row (ky*3 + kx)*3 + ci
  const int dy = tap / 3 - 1, dx = tap - 3 * (tap / 3) - 1;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  ymi_pos_walk at(pos0 + kk, p.W, p.H);                // this lane's positions: pos0 + kk, + 2, + 4, ..
  // element offsets fit 32 bits (validate_preconv_wgrad)
  const float *xb = p.x, *gb = p.g;

  struct Grp { float a[PW_G]; float b[PW_G]; unsigned am; };
  auto issue = [&](Grp &G) {
    G.am = 0u;
#pragma unroll
    for (int s = 0; s < PW_G; ++s) {
      const bool live = at.pos < pos1;
      const int iy = at.oy + dy, ix = at.ox + dx;
      const bool inside = live && row_used && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      G.am |= (inside ? 1u : 0u) << s;
      // the lane's own element: pixel (n, iy, ix), channel ci; element 0 where it is masked (never read out of bounds)
      const unsigned xo = inside ? (unsigned)(((at.n * p.H + iy) * p.W + ix) * 4 + ci) : 0u;
      G.a[s] = xb[xo];
      // a position past the chunk loads nothing and contributes 0
      const unsigned gi = (unsigned)at.pos * (unsigned)p.ldg + (unsigned)(ob + ln);
      G.b[s] = live ? gb[gi] : 0.f;
      at.step2(p.W, p.H);
    }
  };
  auto consume = [&](const Grp &G) {
#pragma unroll
    for (int s = 0; s < PW_G; ++s) {
      const float a = (G.am >> s & 1u) ? G.a[s] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, G.b[s], acc, 0, 0, 0);
    }
  };
  Grp G0, G1;
  issue(G0);
  for (long m0 = pos0; m0 < pos1; m0 += 4 * PW_G) {
    issue(G1);                                         // (past the chunk: every mask bit is 0)
    consume(G0);
    issue(G0);
    consume(G1);
  }

  // accumulator row = row of dw; every element of this chunk's [27, Cout] partial is written once
  float *dst = p.ws + (size_t)blockIdx.y * PW_K * p.Cout;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = ymi_acc_row(r, kk);
    if (row < PW_K) dst[(size_t)row * p.Cout + ob + ln] = acc[r];
  }
#endif
}

// thread = one element of dw [27, Cout]
__global__ __launch_bounds__(256) void preconv_wgrad_sum_k(const PwParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x, nw = (long)PW_K * p.Cout;
  if (i >= nw) return;
  p.dw[i] = ymi_chunk_sum(p.ws, nw, p.nchunks, i);
}

inline long preconv_positions(const ymi_preconv_wgrad_desc *d) { return (long)d->B * d->H * d->W; }

int validate_preconv_wgrad(const ymi_preconv_wgrad_desc *d) {
  if (!d) return YMI_ENULL;
  if (d->B < 1 || d->H < 1 || d->W < 1 || d->Cout < 1) return YMI_EARG;
  if (d->Cout % 32 != 0 || d->ldg < d->Cout || d->ldg % 4 != 0) return YMI_ESHAPE;
  if (preconv_positions(d) * 4 >= (1L << 29) || preconv_positions(d) * d->ldg >= (1L << 29)) return YMI_ESHAPE;
  if (d->Cout / 32 > 65535) return YMI_ESHAPE;
  return YMI_OK;
}

// the chunks of a validated shape: about 2048 one-wave blocks over the Cout / 32 channel groups
ymi_chunks preconv_wgrad_plan(const ymi_preconv_wgrad_desc *d) { return ymi_chunk_plan(preconv_positions(d), 2048, d->Cout / 32); }

}  // namespace

// Workspace of ymi_preconv_wgrad_nhwc_f32: [nchunks][27][Cout] floats
extern "C" int64_t ymi_preconv_wgrad_ws_bytes(const ymi_preconv_wgrad_desc *d) {
  const int rc = validate_preconv_wgrad(d);
  if (rc) return rc;
  return ymi_ws_part((int64_t)preconv_wgrad_plan(d).nchunks * PW_K * d->Cout);
}

extern "C" int ymi_preconv_wgrad_nhwc_f32(const ymi_preconv_wgrad_desc *d, void *stream) {
  const int rc = validate_preconv_wgrad(d);
  if (rc) return rc;
  if (!d->x || !d->g || !d->dw || !d->ws) return YMI_ENULL;
  if ((uintptr_t)d->ws & 15) return YMI_ESHAPE;
  if (d->ws_bytes < ymi_preconv_wgrad_ws_bytes(d)) return YMI_ESHAPE;
  PwParams p;
  p.x = d->x; p.g = d->g; p.dw = d->dw; p.ws = static_cast<float *>(d->ws);
  p.H = d->H; p.W = d->W; p.Cout = d->Cout; p.ldg = d->ldg;
  const ymi_chunks c = preconv_wgrad_plan(d);
  p.P = preconv_positions(d); p.per = c.per; p.nchunks = c.nchunks;
  int rl = ymi_launch(preconv_wgrad_k, dim3(1, p.nchunks, d->Cout / 32), dim3(64), 0, stream, p);
  if (!rl) rl = ymi_launch(preconv_wgrad_sum_k, dim3((unsigned)(((long)PW_K * d->Cout + 255) / 256)), dim3(256), 0, stream, p);
  return rl;
}
