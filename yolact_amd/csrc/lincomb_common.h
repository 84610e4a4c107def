// Shared by the two lincomb terms (mask_loss.hip, maskiou_loss.hip): x = sum_k proto[b,r,c,k] * coef[j,k], p = sigmoid(x), cropped
// to instance j's window, and the backward of a per-pixel term of p to proto and coef in one pass (ymi_lincomb_bwd).
//
// ymi_lincomb_bwd: grid (pixel tiles, images), 256 threads, one thread = one pixel of a 256-pixel tile.  The pixel's 32 prototype
// values and its 32 d_proto accumulators live in registers for the whole launch; the image's coefficient rows and crop windows (and
// what the term stages next to them) are staged in LDS, up to `cap` instances at once and more in further rounds, and read as
// broadcasts.  A logit is consumed where it is produced: nothing of size mh*mw*n exists.  Per instance a wave reduces its 64 values
// of g * proto[k] (a register transpose-reduce: 32 shuffles for the 32 channels, lane 2k ends up with channel k), the four waves are
// combined in a fixed order through LDS every JC instances, and the tile's partial goes to the workspace row [tile][j][32]; the
// term's own *_dcoef_k then adds the tile partials in tile order.  A wave none of whose pixels lies inside the instance's crop window
// skips the dot product and the exp (g = 0 there).  No floating-point atomics anywhere: the same inputs give the same bits, and like
// loss_common.h's sums nothing below may be re-associated (the fmaf chains run k ascending).  Every thread reaches every barrier: one
// before and one after a round's staging, two per JC group; the break inside a group is block-uniform, the skip wave-uniform.
//
// A term is a small struct the skeleton constructs per thread, Term(p, staged, tail):
//   STAGED, TAIL        floats of LDS it wants per staged instance (after the windows) and once (after the per-wave sums)
//   crop()              whether the window is the box's (else the whole map)
//   stage(i, j)         fills its staged values of slot i from instance j
//   pixel(jj, pix, ok)  starts a pixel of staged instance jj (before the window test)
//   grad(x, s, j, pix)  g = d term / d x of a pixel inside the window, from the logit and its sigmoid split
//   mult(g, jj)         what multiplies coef[k] in the d_proto update (the transpose-reduce takes g itself)
//   instance_end(u)     after instance u of a JC group (every thread reaches it)
//   combine(row, u)     thread (u, k = 0) of the combine step, row = tile * N + j
//
// Numerics.  With e = exp(-|x|), r = 1 / (1 + e): p = r or e r, 1 - p = e r or r (no cancellation; ymi_sigmoid_split), finite for any
// finite x.
#pragma once
#include "loss_common.h"

constexpr int YMI_LINCOMB_TP = 256;      // pixels per block (one per thread)
constexpr int YMI_LINCOMB_JC = 8;        // instances between two cross-wave combines: JC * 32 = 256 sums, one per thread

// sanitize_coordinates(_x1, _x2, img_size, padding=1, cast=False) in both directions: x1, x2, y1, y2
__device__ __forceinline__ f32x4 ymi_crop_window(const float *b4, int mh, int mw) {
  const float a = b4[0] * (float)mw, c = b4[2] * (float)mw;
  float x1 = fminf(a, c) - 1.f; x1 = x1 < 0.f ? 0.f : x1;
  float x2 = fmaxf(a, c) + 1.f; x2 = x2 > (float)mw ? (float)mw : x2;
  const float d = b4[1] * (float)mh, e = b4[3] * (float)mh;
  float y1 = fminf(d, e) - 1.f; y1 = y1 < 0.f ? 0.f : y1;
  float y2 = fmaxf(d, e) + 1.f; y2 = y2 > (float)mh ? (float)mh : y2;
  return f32x4{x1, x2, y1, y2};
}

__device__ __forceinline__ bool ymi_in_window(const f32x4 w4, float fx, float fy) {
  return fx >= w4[0] && fx < w4[1] && fy >= w4[2] && fy < w4[3];
}

// a GT row index nobody validated on the device
__device__ __forceinline__ int ymi_clamp_row(int g, int G) { return g < 0 ? 0 : (g >= G ? G - 1 : g); }

struct ymi_sigmoid { float e, p, om; };   // exp(-|x|), sigmoid(x), 1 - sigmoid(x)
__device__ __forceinline__ ymi_sigmoid ymi_sigmoid_split(float x) {
  const float e = expf(-fabsf(x));
  const float r = 1.f / (1.f + e), er = e * r;
  return ymi_sigmoid{e, x >= 0.f ? r : er, x >= 0.f ? er : r};
}

// a pixel's 32 channels (16-byte accesses; zeros for a pixel past the map, whose src is any valid pixel)
__device__ __forceinline__ void ymi_load32(const float *src, bool ok, float (&P)[32]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f32x4 v = *reinterpret_cast<const f32x4 *>(src + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) P[4 * q + e] = ok ? v[e] : 0.f;
  }
}
__device__ __forceinline__ void ymi_store32(float *dst, const float (&dp)[32]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = dp[4 * q + e];
    *reinterpret_cast<f32x4 *>(dst + 4 * q) = v;
  }
}

// transpose-reduce of v[k] = g * P[k] over the wave: at distance m = 32, 16, .., 2 a lane keeps the upper or the lower half of its
// values (by its bit m) and receives the partner's sums of that half; after five steps lane l holds channel l >> 1 summed over the
// 32 lanes that share its bit 0, the last step adds the other 32.  Every lane of the wave calls it; lane 2k returns channel k.
__device__ __forceinline__ float ymi_transpose_reduce32(float g, const float (&P)[32], int lane) {
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
  return v[0] + __shfl_xor(v[0], 1);
}

// P: proto, coef, box, img_off, d_proto, ws_dc [ntiles][N][32], mh, mw, npix, N, cap, want_dc.  lds: ymi_lincomb_lds<Term>() bytes.
template <class Term, class P> __device__ __forceinline__ void ymi_lincomb_bwd(const P &p, float *lds) {
  constexpr int JC = YMI_LINCOMB_JC;
  float *cs = lds;                                   // [cap][32] coefficient rows
  float *win = cs + p.cap * 32;                      // [cap][4]  crop window x1, x2, y1, y2
  float *staged = win + p.cap * 4;                   // [cap][STAGED] the term's
  float *red = staged + p.cap * Term::STAGED;        // [4][JC][32] per-wave sums of g * proto[k]
  Term term(p, staged, red + 4 * JC * 32);           // [TAIL] the term's

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.y, tile = blockIdx.x;
  const int pix = tile * YMI_LINCOMB_TP + t;
  const bool ok = pix < p.npix;
  const int py = ok ? pix / p.mw : 0, px = ok ? pix - py * p.mw : 0;
  const float fx = (float)px, fy = (float)py;

  int j0, nj;
  ymi_image_range(p.img_off, b, p.N, j0, nj);
  const int j1 = j0 + nj;

  float P32[32], dp[32];
  ymi_load32(p.proto + ((size_t)b * p.npix + (ok ? pix : 0)) * 32, ok, P32);
#pragma unroll
  for (int k = 0; k < 32; ++k) dp[k] = 0.f;

  for (int c0 = j0; c0 < j1; c0 += p.cap) {
    const int cnt = j1 - c0 < p.cap ? j1 - c0 : p.cap;
    __syncthreads();                                 // the previous round's rows have been read
    for (int i = t; i < cnt * 32; i += 256) cs[i] = p.coef[(size_t)c0 * 32 + i];
    for (int i = t; i < cnt; i += 256) {
      const int j = c0 + i;
      *reinterpret_cast<f32x4 *>(win + 4 * i) =
          term.crop() ? ymi_crop_window(p.box + (size_t)j * 4, p.mh, p.mw) : f32x4{0.f, (float)p.mw, 0.f, (float)p.mh};
      term.stage(i, j);
    }
    __syncthreads();

    for (int jj0 = 0; jj0 < cnt; jj0 += JC) {
#pragma unroll 1
      for (int u = 0; u < JC; ++u) {
        const int jj = jj0 + u;
        if (jj >= cnt) break;                        // block-uniform
        const float *c = cs + jj * 32;
        const f32x4 w4 = *reinterpret_cast<const f32x4 *>(win + 4 * jj);
        term.pixel(jj, pix, ok);
        const bool inside = ok && ymi_in_window(w4, fx, fy);
        float g = 0.f;
        const bool any_in = __any(inside) != 0;      // wave-uniform
        if (any_in) {
          float x = 0.f;
#pragma unroll
          for (int k = 0; k < 32; ++k) x = fmaf(P32[k], c[k], x);
          const ymi_sigmoid s = ymi_sigmoid_split(x);
          if (inside) g = term.grad(x, s, c0 + jj, pix);
          const float gs = term.mult(g, jj);
#pragma unroll
          for (int k = 0; k < 32; ++k) dp[k] = fmaf(gs, c[k], dp[k]);
        }
        term.instance_end(u);
        if (p.want_dc) {
          float v0 = 0.f;
          if (any_in) v0 = ymi_transpose_reduce32(g, P32, lane);
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
          if (k == 0) term.combine(row, u);
        }
      }
      __syncthreads();
    }
  }

  if (p.d_proto && ok) ymi_store32(p.d_proto + ((size_t)b * p.npix + pix) * 32, dp);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static inline int ymi_lincomb_ntiles(int mh, int mw) { return (mh * mw + YMI_LINCOMB_TP - 1) / YMI_LINCOMB_TP; }

// cap = instances staged at once: N rounded up to a JC group, at most the kernel's cap_max (N = 0 still names a group); returns the
// dynamic LDS bytes of ymi_lincomb_bwd<Term> at that cap
template <class Term> static inline size_t ymi_lincomb_lds(int N, int cap_max, int &cap) {
  const int n8 = (N + 7) / 8 * 8;
  cap = n8 < 8 ? 8 : (n8 > cap_max ? cap_max : n8);
  return ((size_t)cap * (32 + 4 + Term::STAGED) + 4 * YMI_LINCOMB_JC * 32 + Term::TAIL) * sizeof(float);
}
