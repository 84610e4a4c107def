// The backward of the train-mode ResNet stem (backbone.py:129-132: conv1 7x7 / 2 / pad 3 on 3 channels, bn1, ReLU, MaxPool2d(3, 2, 1)),
// NHWC fp32, without atomics (the same inputs give the same bits).  The forward convolution runs on ymi_conv2d_nhwc_f32 (the Cin-4
// loader), BatchNorm + ReLU on csrc/bn_train.hip; what is new here:
//
//   ymi_stem_wgrad_nhwc_f32     dw[k,co] = sum_pos x[n, 2 oy + ky - 3, 2 ox + kx - 3, ci] g[pos,co], k = (ky*7 + kx)*3 + ci, in the structure
//                               of grad_common.h (positions = the matrix instruction's k index, chunk partials, an ordered sum).
//                               x is the NHWC-4 image the forward reads, so for one output pixel and one ky the 8 pixels from
//                               column 2 ox - 3 on are 32 CONSECUTIVE floats: the rows (kx, c4) of one 32-row tile, of which kx = 7 and
//                               c4 = 3 are discarded (28 * 3 / 4 = 21 of 32 rows are used); the B operand is 32 consecutive channels
//                               of g.  A block owns a chunk of positions and 64 output channels; its wave w owns ky = w and
//                               ky = w + 4 (wave 3: ky = 3 alone), at most 2 x 2 accumulator tiles = 64 registers.  A lane outside the
//                               image (left / right border, a row above or below), in a discarded row or past the chunk is masked
//                               to 0 by a select, never by a product, so the padding channel may hold anything.
//   ymi_maxpool_fwd_nhwc_f32    3x3 / 2 / pad 1, -inf outside, `v > m ? v : m` in row-major window order.
//   ymi_maxpool_bwd_nhwc_f32    a gather: an input pixel looks at the 1, 2, 2 or 4 windows that hold it (by its row and column parity),
//                               RECOMPUTES each window's argmax from x (greater than everything before it in row-major window order,
//                               not smaller than anything after it: the first of equal maxima) and adds dy where it is its own.
#include "grad_common.h"
#include "../../include/yolact_amd.h"

namespace {

// ---- weight gradient of the stem convolution -------------------------------------------------------------------------------------------
struct SwParams {
  const float *x, *g;
  float *dw, *ws;
  int H, W, Ho, Wo, Cout, ldg, nchunks;
  long P, per;
};

constexpr int SW_K = 147;                              // 7 * 7 * 3 rows of dw
constexpr int SW_G = 8;                                // instructions per load group (16 positions)

__global__ __launch_bounds__(256, 2) void stem_wgrad_k(const SwParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ln = lane & 31, kk = lane >> 5;
  const int nky = wave + 4 < 7 ? 2 : 1;                // ky = wave, wave + 4
  const int ob = blockIdx.z * 64;
  const int nct = p.Cout - ob >= 64 ? 2 : 1;           // 32-column tiles of this block that hold real channels (Cout % 32 == 0)
  const long pos0 = (long)blockIdx.y * p.per;
  const long pos1 = pos0 + p.per < p.P ? pos0 + p.per : p.P;
  const bool row_used = ln < 28 && (ln & 3) != 3;      // kx < 7 and not the padding channel
  const int dxl = ln >> 2;                             // this lane's pixel within the 8 of a row tile

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  ymi_pos_walk at(pos0 + kk, p.Wo, p.Ho);      // this lane's positions: pos0 + kk, + 2, + 4, ..
  // element offsets fit 32 bits (validate_stem_wgrad)
  const float *xb = p.x, *gb = p.g;

  struct Grp { float a[2][SW_G]; float b[2][SW_G]; unsigned am[2]; };
  auto issue = [&](Grp &G) {
    G.am[0] = 0u; G.am[1] = 0u;
#pragma unroll
    for (int s = 0; s < SW_G; ++s) {
      const bool live = at.pos < pos1;
      const int ix = 2 * at.ox - 3 + dxl;
      const bool colok = live && row_used && (unsigned)ix < (unsigned)p.W;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int iy = 2 * at.oy + wave + 4 * i - 3;
        const bool inside = i < nky && colok && (unsigned)iy < (unsigned)p.H;
        G.am[i] |= (inside ? 1u : 0u) << s;
        // the lane's own element: pixel (n, iy, ix), channel ln & 3; element 0 where it is masked (never read out of bounds)
        const unsigned xo = inside ? (unsigned)(((at.n * p.H + iy) * p.W + ix) * 4 + (ln & 3)) : 0u;
        G.a[i][s] = i < nky ? xb[xo] : 0.f;
      }
      // a position past the chunk loads nothing and contributes 0
      const unsigned gi = (unsigned)at.pos * (unsigned)p.ldg + (unsigned)(ob + ln);
#pragma unroll
      for (int j = 0; j < 2; ++j) G.b[j][s] = (j < nct && live) ? gb[gi + 32u * j] : 0.f;
      at.step2(p.Wo, p.Ho);
    }
  };
  auto consume = [&](const Grp &G) {
#pragma unroll
    for (int s = 0; s < SW_G; ++s) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j < nct) {
          const float b = G.b[j][s];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            if (i < nky) {
              const float a = (G.am[i] >> s & 1u) ? G.a[i][s] : 0.f;
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i][j], 0, 0, 0);
            }
          }
        }
      }
    }
  };
  Grp G0, G1;
  issue(G0);
  for (long m0 = pos0; m0 < pos1; m0 += 4 * SW_G) {
    issue(G1);                                         // (past the chunk: every mask bit is 0)
    consume(G0);
    issue(G0);
    consume(G1);
  }

  // accumulator row (kx, c4) -> row (ky*7 + kx)*3 + c of dw; every element of this chunk's [147, Cout] partial is written once
  float *dst = p.ws + (size_t)blockIdx.y * SW_K * p.Cout;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (i < nky) {
      const int ky = wave + 4 * i;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j < nct) {
          const int o = ob + 32 * j + ln;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = ymi_acc_row(r, kk), kx = row >> 2, c = row & 3;
            if (kx < 7 && c < 3) dst[(size_t)((ky * 7 + kx) * 3 + c) * p.Cout + o] = acc[i][j][r];
          }
        }
      }
    }
  }
#endif
}

// thread = one element of dw [147, Cout]
__global__ __launch_bounds__(256) void stem_wgrad_sum_k(const SwParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x, nw = (long)SW_K * p.Cout;
  if (i >= nw) return;
  p.dw[i] = ymi_chunk_sum(p.ws, nw, p.nchunks, i);
}

inline int stem_out(int size) { return (size - 1) / 2 + 1; }
inline long stem_positions(const ymi_stem_wgrad_desc *d) { return (long)d->B * stem_out(d->H) * stem_out(d->W); }

int validate_stem_wgrad(const ymi_stem_wgrad_desc *d) {
  if (!d) return YMI_ENULL;
  if (d->B < 1 || d->H < 1 || d->W < 1 || d->Cout < 1) return YMI_EARG;
  if (d->Cout % 32 != 0 || d->ldg < d->Cout || d->ldg % 4 != 0) return YMI_ESHAPE;
  if ((long)d->B * d->H * d->W * 4 >= (1L << 29) || stem_positions(d) * d->ldg >= (1L << 29)) return YMI_ESHAPE;
  if ((d->Cout + 63) / 64 > 65535) return YMI_ESHAPE;
  return YMI_OK;
}

// the chunks of a validated shape: about 512 blocks over the ceil(Cout / 64) channel groups
ymi_chunks stem_wgrad_plan(const ymi_stem_wgrad_desc *d) { return ymi_chunk_plan(stem_positions(d), 512, (d->Cout + 63) / 64); }

// ---- max-pool 3x3 / 2 / pad 1 ------------------------------------------------------------------------------------------------------------
struct MpParams {
  const float *x, *dy;
  float *y, *dx;
  int H, W, C4, Hp, Wp;
  long total;
};

// thread = (output pixel, 4 channels)
__global__ __launch_bounds__(256) void maxpool_fwd_k(const MpParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const int c4 = (int)(i % p.C4);
  long r = i / p.C4;
  const int ox = (int)(r % p.Wp); r /= p.Wp;
  const int oy = (int)(r % p.Hp);
  const long b = r / p.Hp;
  const float ninf = -__builtin_inff();
  f32x4 m = {ninf, ninf, ninf, ninf};
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy - 1 + ky;
    if ((unsigned)iy >= (unsigned)p.H) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox - 1 + kx;
      if ((unsigned)ix >= (unsigned)p.W) continue;
      const f32x4 v = *reinterpret_cast<const f32x4 *>(p.x + ((((size_t)b * p.H + iy) * p.W + ix) * p.C4 + c4) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
    }
  }
  *reinterpret_cast<f32x4 *>(p.y + (size_t)i * 4) = m;
}

// thread = (input pixel, 4 channels); windows with output rows ascending, within a row output columns ascending
__global__ __launch_bounds__(256) void maxpool_bwd_k(const MpParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const int c4 = (int)(i % p.C4);
  long r = i / p.C4;
  const int ix = (int)(r % p.W); r /= p.W;
  const int iy = (int)(r % p.H);
  const long b = r / p.H;
  const f32x4 me = *reinterpret_cast<const f32x4 *>(p.x + (size_t)i * 4);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // the windows that hold row iy: oy = iy / 2 for an even row, (iy - 1) / 2 and (iy + 1) / 2 for an odd one
  const int oy0 = iy >> 1, oy1 = (iy + 1) >> 1, ox0 = ix >> 1, ox1 = (ix + 1) >> 1;
  for (int oy = oy0; oy <= oy1; ++oy) {
    if (oy >= p.Hp) continue;
    for (int ox = ox0; ox <= ox1; ++ox) {
      if (ox >= p.Wp) continue;
      const int mine = (iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1));   // this pixel's place in the window, row-major
      bool win[4] = {true, true, true, true};
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int wy = 2 * oy - 1 + ky;
        if ((unsigned)wy >= (unsigned)p.H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int wx = 2 * ox - 1 + kx, at = ky * 3 + kx;
          if ((unsigned)wx >= (unsigned)p.W || at == mine) continue;
          const f32x4 v = *reinterpret_cast<const f32x4 *>(p.x + ((((size_t)b * p.H + wy) * p.W + wx) * p.C4 + c4) * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) win[e] = win[e] && (at < mine ? me[e] > v[e] : me[e] >= v[e]);
        }
      }
      const f32x4 d = *reinterpret_cast<const f32x4 *>(p.dy + ((((size_t)b * p.Hp + oy) * p.Wp + ox) * p.C4 + c4) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += win[e] ? d[e] : 0.f;
    }
  }
  *reinterpret_cast<f32x4 *>(p.dx + (size_t)i * 4) = acc;
}

int validate_maxpool(int B, int H, int W, int C) {
  if (B < 1 || H < 1 || W < 1 || C < 1) return YMI_EARG;
  if (C % 4 != 0 || (double)B * H * W * C >= 0x1p40) return YMI_ESHAPE;
  return YMI_OK;
}

}  // namespace

// Workspace of ymi_stem_wgrad_nhwc_f32: [nchunks][147][Cout] floats
extern "C" int64_t ymi_stem_wgrad_ws_bytes(const ymi_stem_wgrad_desc *d) {
  const int rc = validate_stem_wgrad(d);
  if (rc) return rc;
  return ymi_ws_part((int64_t)stem_wgrad_plan(d).nchunks * SW_K * d->Cout);
}

extern "C" int ymi_stem_wgrad_nhwc_f32(const ymi_stem_wgrad_desc *d, void *stream) {
  const int rc = validate_stem_wgrad(d);
  if (rc) return rc;
  if (!d->x || !d->g || !d->dw || !d->ws) return YMI_ENULL;
  if ((uintptr_t)d->ws & 15) return YMI_ESHAPE;
  if (d->ws_bytes < ymi_stem_wgrad_ws_bytes(d)) return YMI_ESHAPE;
  SwParams p;
  p.x = d->x; p.g = d->g; p.dw = d->dw; p.ws = static_cast<float *>(d->ws);
  p.H = d->H; p.W = d->W; p.Ho = stem_out(d->H); p.Wo = stem_out(d->W); p.Cout = d->Cout; p.ldg = d->ldg;
  const ymi_chunks c = stem_wgrad_plan(d);
  p.P = stem_positions(d); p.per = c.per; p.nchunks = c.nchunks;
  int rl = ymi_launch(stem_wgrad_k, dim3(1, p.nchunks, (d->Cout + 63) / 64), dim3(256), 0, stream, p);
  if (!rl) rl = ymi_launch(stem_wgrad_sum_k, dim3((unsigned)(((long)SW_K * d->Cout + 255) / 256)), dim3(256), 0, stream, p);
  return rl;
}

extern "C" int ymi_maxpool_fwd_nhwc_f32(const float *x, float *y, int B, int H, int W, int C, void *stream) {
  if (!x || !y) return YMI_ENULL;
  const int rc = validate_maxpool(B, H, W, C);
  if (rc) return rc;
  if (((uintptr_t)x | (uintptr_t)y) & 15) return YMI_ESHAPE;
  MpParams p;
  p.x = x; p.dy = nullptr; p.y = y; p.dx = nullptr; p.H = H; p.W = W; p.C4 = C / 4; p.Hp = (H - 1) / 2 + 1; p.Wp = (W - 1) / 2 + 1;
  p.total = (long)B * p.Hp * p.Wp * p.C4;
  return ymi_launch(maxpool_fwd_k, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, stream, p);
}

extern "C" int ymi_maxpool_bwd_nhwc_f32(const float *x, const float *dy, float *dx, int B, int H, int W, int C, void *stream) {
  if (!x || !dy || !dx) return YMI_ENULL;
  const int rc = validate_maxpool(B, H, W, C);
  if (rc) return rc;
  if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) return YMI_ESHAPE;
  MpParams p;
  p.x = x; p.dy = dy; p.y = nullptr; p.dx = dx; p.H = H; p.W = W; p.C4 = C / 4; p.Hp = (H - 1) / 2 + 1; p.Wp = (W - 1) / 2 + 1;
  p.total = (long)B * H * W * p.C4;
  return ymi_launch(maxpool_bwd_k, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, stream, p);
}
