// DCNv2 backward (external/DCNv2/src/cuda/dcn_v2_cuda.cu:174-335, dcn_v2_im2col_cuda.cu:197-327) for the geometry the forward of
// csrc/dcn.hip takes: 3x3, padding 1, dilation 1, one deformable group, square stride 1 or 2, NHWC fp32, Cin % 32 == 0.
//
// Notation: m = output pixel (b, oy, ox), tap k = 3i + j, sample point (h, w) = (oy*s - 1 + i) + dh_k, (ox*s - 1 + j) + dw_k formed in
// fp32 exactly as the forward forms it, mu_k the modulation, S_k[c] the zero-padded bilinear sample of x[b, :, :, c] at (h, w),
// gcol[m,k,c] = sum_o W[o,k,c] * gy[m,o].
//     gx[b,y,x,c] += corner weight * mu_k * gcol[m,k,c]        for the (up to four) corners of the point that lie inside the image
//     gmu[m,k]     = sum_c gcol[m,k,c] * S_k[c]
//     gdh[m,k]     = mu_k * sum_c gcol[m,k,c] * dS_k[c]/dh     (gdw likewise); corners outside the image contribute 0, and all three
//                    are exactly 0 when the point is outside -1 < h < H, -1 < w < W
//     gW[o,k,c]    = sum_m gy[m,o] * mu_k * S_k[c]
//     gbias[o]     = sum_m gy[m,o]
//
// Two kernels, both on the exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32: fp32 in, fp32 accumulate), both FUSED — neither
// gcol nor the column tensor (each 9x the activation) exists in memory:
//   * dcn_bwd_data_k: a block owns 32 output pixels.  Per tap its four waves take the 32-channel chunks round robin; a wave forms
//     the 32 x 32 gcol tile (gy tile from LDS x filter rows straight from L2) in 16 accumulator registers, and while the tile is in
//     registers — one register = one pixel row pair, lane = channel — gathers the four corners of x (two 128-byte segments per
//     load), accumulates gmu / gdh / gdw per pixel, and adds corner weight * mu * gcol into gx with fp32 atomics (no-return
//     global_atomic_add_f32, two 128-byte segments per wave instruction: the shape the memory-side atomic units take at full
//     rate).  The per-pixel sums are reduced over the lanes, then over the waves through LDS in a fixed order and stored; only when
//     the channel chunks of small maps are spread over several blocks (gridDim.y > 1) are they combined with atomics too.
//   * dcn_bwd_weight_k: a block owns one (tap, 32-channel chunk) and a range of m.  Per 32 pixels it rebuilds the modulated column
//     tile in LDS (the forward's gather: four 16-byte corner loads per 4 channels), every wave multiplies gy^T by it for its share
//     of the output channels, and the ranges are combined with fp32 atomics into gW.  gbias falls out of the gy fragments of the
//     blocks of (tap 0, chunk 0).
// The sampling geometry (dcn_point) restates the arithmetic of the `geom` lambda of csrc/dcn.hip, which is closed over that
// kernel's register state and cannot be called from here; tests/test_gpu_dcn_bwd.py holds the two to the same fp64 reference.
//
// NOT bit-reproducible from run to run: gx, gW, gbias (and goff / gmask on small maps) are sums of float atomics, whose order of
// arrival varies.  The error of any order is that of an fp32 sum of the same terms.
#include "grad_common.h"
#include "../../include/yolact_amd.h"

namespace {

struct BwdParams {
  const float *x, *offmask, *w, *gy;
  float *gx, *goff, *gmask, *gw, *gbias;
  int B, H, W, Cin, ldx, Ho, Wo, Cout, stride, ldo, om_layout;
  int M, HoWo;
  int ncc, cc_per_blk, atomic_om;     // data kernel: 32-channel chunks, chunks per block (gridDim.y ranges)
  int m_per_blk;                      // weight kernel: pixels per block (a multiple of 32)
};

// One sample point: element offset of its top-left corner in x (meaningful only for corners whose bit is set), which of the four
// corners (bit 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right) lie inside the image — none when the point is outside
// -1 < h < H, -1 < w < W or m is past the end — the fractions and the modulation.
struct Pt { int o1; unsigned fl; float lh, lw, mk; };

__device__ __forceinline__ Pt dcn_point(const BwdParams &p, int m, int tap) {
  Pt g;
  g.o1 = 0; g.fl = 0u; g.lh = 0.f; g.lw = 0.f; g.mk = 0.f;
  if (m >= p.M) return g;
  const int b = m / p.HoWo, pix = m - b * p.HoWo;
  const int oy = pix / p.Wo, ox = pix - oy * p.Wo;
  const float *om = p.offmask + (size_t)m * p.ldo;
  float dh, dw;
  if (p.om_layout) { dh = om[3 * tap]; dw = om[3 * tap + 1]; g.mk = om[3 * tap + 2]; }
  else { dh = om[2 * tap]; dw = om[2 * tap + 1]; g.mk = om[18 + tap]; }
  const int ky = tap / 3, kx = tap - 3 * ky;
  const float h = (float)(oy * p.stride - 1 + ky) + dh, w = (float)(ox * p.stride - 1 + kx) + dw;
  const bool in = h > -1.f && w > -1.f && h < (float)p.H && w < (float)p.W;
  if (!in) return g;
  const int hl = (int)floorf(h), wl = (int)floorf(w);
  g.lh = h - (float)hl; g.lw = w - (float)wl;
  g.o1 = ((b * p.H + hl) * p.W + wl) * p.ldx;
  const bool t_ = hl >= 0, b_ = hl + 1 <= p.H - 1, l_ = wl >= 0, r_ = wl + 1 <= p.W - 1;
  g.fl = (unsigned)(t_ && l_) | ((unsigned)(t_ && r_) << 1) | ((unsigned)(b_ && l_) << 2) | ((unsigned)(b_ && r_) << 3);
  return g;
}

__global__ __launch_bounds__(256) void dcn_bwd_data_k(const BwdParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  __shared__ float As[32 * 33];                      // gy tile, transposed: As[o][pixel], 33-float rows (conflict-free both ways)
  __shared__ int g_o1[32];
  __shared__ unsigned g_fl[32];
  __shared__ float g_lh[32], g_lw[32], g_mk[32];
  __shared__ float red[3][4][32];                    // per-wave partial gmu / gdh / gdw of the block's 32 pixels
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ln = lane & 31, kk = lane >> 5;
  const int m0 = blockIdx.x * 32;
  const int cc0 = blockIdx.y * p.cc_per_blk;
  const int cc1 = cc0 + p.cc_per_blk < p.ncc ? cc0 + p.cc_per_blk : p.ncc;
  const int nci = (cc1 - cc0 + 3) / 4;               // trips of the chunk loop: the same for every wave (barriers inside)
  const bool want_om = p.goff != nullptr || p.gmask != nullptr;
  const int sr = t >> 3, so4 = (t & 7) * 4;          // staging: pixel row, first of four output channels
  const int dx = p.ldx, dy = p.W * p.ldx;

  for (int tap = 0; tap < 9; ++tap) {
    __syncthreads();                                 // the previous tap's geometry and partial sums have been read
    if (t < 32) {
      const Pt g = dcn_point(p, m0 + t, tap);
      g_o1[t] = g.o1; g_fl[t] = g.fl; g_lh[t] = g.lh; g_lw[t] = g.lw; g_mk[t] = g.mk;
    }
    float pm[16], ph[16], pw[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { pm[r] = 0.f; ph[r] = 0.f; pw[r] = 0.f; }

    for (int ci = 0; ci < nci; ++ci) {
      const int cc = cc0 + 4 * ci + wave;
      const bool act = cc < cc1;
      const int c0 = cc * 32;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      for (int o0 = 0; o0 < p.Cout; o0 += 32) {
        __syncthreads();                             // every wave is done with the previous gy tile
        {
          const int m = m0 + sr, o = o0 + so4;
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (m < p.M) {
            const float *src = p.gy + (size_t)m * p.Cout + o;
            if ((p.Cout & 3) == 0 && o + 3 < p.Cout) {
              v = *reinterpret_cast<const f32x4 *>(src);
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (o + e < p.Cout) v[e] = src[e];
            }
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) As[(so4 + e) * 33 + sr] = v[e];
        }
        __syncthreads();
        if (act) {
          const float *wp = p.w + ((size_t)(o0 + kk) * 9 + tap) * p.Cin + c0 + ln;
          float bv[16];
#pragma unroll
          for (int s = 0; s < 16; ++s) bv[s] = (o0 + 2 * s + kk < p.Cout) ? wp[(size_t)(2 * s) * 9 * p.Cin] : 0.f;
#pragma unroll
          for (int s = 0; s < 16; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * s + kk) * 33 + ln], bv[s], acc, 0, 0, 0);
        }
      }
      if (act) {
        // the gcol tile is in registers: register r = pixel ymi_acc_row(r, kk), lane = channel c0 + ln
        const float *xc = p.x + c0 + ln;
        float *gxc = p.gx ? p.gx + c0 + ln : nullptr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = ymi_acc_row(r, kk);
          const unsigned fl = g_fl[i];
          if (fl) {
            const int o1 = g_o1[i];
            const float lh = g_lh[i], lw = g_lw[i], uh = 1.f - lh, uw = 1.f - lw;
            const float g = acc[r];
            if (want_om) {
              const float v0 = (fl & 1u) ? xc[o1] : 0.f, v1 = (fl & 2u) ? xc[o1 + dx] : 0.f;
              const float v2 = (fl & 4u) ? xc[o1 + dy] : 0.f, v3 = (fl & 8u) ? xc[o1 + dy + dx] : 0.f;
              const float S = (uh * uw) * v0 + (uh * lw) * v1 + (lh * uw) * v2 + (lh * lw) * v3;
              pm[r] += g * S;
              ph[r] += g * (uw * (v2 - v0) + lw * (v3 - v1));
              pw[r] += g * (uh * (v1 - v0) + lh * (v3 - v2));
            }
            if (gxc) {
              const float gm = g * g_mk[i];
              if (fl & 1u) atomicAdd(gxc + o1, (uh * uw) * gm);
              if (fl & 2u) atomicAdd(gxc + o1 + dx, (uh * lw) * gm);
              if (fl & 4u) atomicAdd(gxc + o1 + dy, (lh * uw) * gm);
              if (fl & 8u) atomicAdd(gxc + o1 + dy + dx, (lh * lw) * gm);
            }
          }
        }
      }
    }

    if (want_om) {
      // sum over the 32 channels a half wave holds, then over the waves (fixed order)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) {
          pm[r] += __shfl_xor(pm[r], d);
          ph[r] += __shfl_xor(ph[r], d);
          pw[r] += __shfl_xor(pw[r], d);
        }
        if (ln == r) {
          const int i = ymi_acc_row(r, kk);
          red[0][wave][i] = pm[r]; red[1][wave][i] = ph[r]; red[2][wave][i] = pw[r];
        }
      }
      __syncthreads();
      if (t < 32 && m0 + t < p.M) {
        const float sm = ((red[0][0][t] + red[0][1][t]) + red[0][2][t]) + red[0][3][t];
        const float sh = ((red[1][0][t] + red[1][1][t]) + red[1][2][t]) + red[1][3][t];
        const float sw = ((red[2][0][t] + red[2][1][t]) + red[2][2][t]) + red[2][3][t];
        const float mk = g_mk[t];
        const size_t m = (size_t)(m0 + t);
        if (p.atomic_om) {
          if (g_fl[t]) {
            if (p.gmask) atomicAdd(p.gmask + m * 9 + tap, sm);
            if (p.goff) { atomicAdd(p.goff + m * 18 + 2 * tap, mk * sh); atomicAdd(p.goff + m * 18 + 2 * tap + 1, mk * sw); }
          }
        } else {
          if (p.gmask) p.gmask[m * 9 + tap] = sm;
          if (p.goff) { p.goff[m * 18 + 2 * tap] = mk * sh; p.goff[m * 18 + 2 * tap + 1] = mk * sw; }
        }
      }
    }
  }
#endif
}

// NT: 32-row output-channel tiles per wave (a block covers NT * 128 output channels, gridDim.z such groups)
template <int NT>
__global__ __launch_bounds__(256) void dcn_bwd_weight_k(const BwdParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  __shared__ __attribute__((aligned(16))) float col[32 * 32];      // modulated column tile: col[pixel][channel]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ln = lane & 31, kk = lane >> 5;
  const int tap = blockIdx.x % 9, c0 = (blockIdx.x / 9) * 32;
  const int ob = blockIdx.z * (NT * 128);
  const int mb0 = blockIdx.y * p.m_per_blk;
  const int mb1 = mb0 + p.m_per_blk < p.M ? mb0 + p.m_per_blk : p.M;
  const bool do_w = p.gw != nullptr;
  const bool do_bias = p.gbias != nullptr && blockIdx.x == 0;
  const int row = t >> 3, ch = (t & 7) * 4;
  const int dx = p.ldx, dy = p.W * p.ldx;

  f32x16 acc[NT];
  float bs[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    bs[j] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  }

  for (int m0 = mb0; m0 < mb1; m0 += 32) {
    if (do_w) {
      __syncthreads();                               // every wave is done with the previous column tile
      const Pt g = dcn_point(p, m0 + row, tap);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (g.fl) {
        const float *xb = p.x + c0 + ch + g.o1;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 v0 = (g.fl & 1u) ? *reinterpret_cast<const f32x4 *>(xb) : z;
        const f32x4 v1 = (g.fl & 2u) ? *reinterpret_cast<const f32x4 *>(xb + dx) : z;
        const f32x4 v2 = (g.fl & 4u) ? *reinterpret_cast<const f32x4 *>(xb + dy) : z;
        const f32x4 v3 = (g.fl & 8u) ? *reinterpret_cast<const f32x4 *>(xb + dy + dx) : z;
        const float uh = 1.f - g.lh, uw = 1.f - g.lw;
        v = ((uh * uw) * v0 + (uh * g.lw) * v1 + (g.lh * uw) * v2 + (g.lh * g.lw) * v3) * g.mk;
      }
      *reinterpret_cast<f32x4 *>(&col[row * 32 + ch]) = v;
      __syncthreads();
    }
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {
      const int m = m0 + 2 * s + kk;
      const float b = do_w ? col[(2 * s + kk) * 32 + ln] : 0.f;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int o = ob + (wave + 4 * j) * 32 + ln;
        const float a = (m < p.M && o < p.Cout) ? p.gy[(size_t)m * p.Cout + o] : 0.f;
        bs[j] += a;
        if (do_w) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[j], 0, 0, 0);
      }
    }
  }

  if (do_w) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = ob + (wave + 4 * j) * 32 + ymi_acc_row(r, kk);
        if (o < p.Cout) atomicAdd(p.gw + ((size_t)o * 9 + tap) * p.Cin + c0 + ln, acc[j][r]);
      }
  }
  if (do_bias) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const float v = bs[j] + __shfl_xor(bs[j], 32);
      const int o = ob + (wave + 4 * j) * 32 + ln;
      if (kk == 0 && o < p.Cout) atomicAdd(p.gbias + o, v);
    }
  }
#endif
}

}  // namespace

extern "C" int ymi_dcn_v2_backward_f32(const ymi_dcn_bwd_desc *d, void *stream) {
  if (!d) return YMI_ENULL;
  // what the forward supports and nothing more
  if (d->kh != 3 || d->kw != 3 || d->pad != 1 || d->dilation != 1 || d->deformable_groups != 1) return YMI_EARG;
  if (d->stride != 1 && d->stride != 2) return YMI_EARG;
  if (d->mask_is_prob != 1 || (d->om_layout != 0 && d->om_layout != 1)) return YMI_EARG;
  if (d->B < 1 || d->H < 1 || d->W < 1 || d->Cin < 32 || d->Cout < 1) return YMI_EARG;
  if (d->Cin % 32 != 0 || d->ldx < d->Cin || (d->ldx & 3) || d->ldo < 27) return YMI_ESHAPE;
  if (d->Ho != (d->H + 2 - 3) / d->stride + 1 || d->Wo != (d->W + 2 - 3) / d->stride + 1) return YMI_ESHAPE;
  const long M = (long)d->B * d->Ho * d->Wo;
  if ((long)d->B * d->H * d->W * d->ldx >= (1L << 31) || M * (long)d->ldo >= (1L << 31) || M * (long)d->Cout >= (1L << 31) ||
      (long)d->Cout * 9 * d->Cin >= (1L << 31))
    return YMI_ESHAPE;
  const bool want_data = d->gx || d->g_offset || d->g_mask, want_w = d->gw || d->gbias;
  if (!want_data && !want_w) return YMI_OK;
  if (!d->gy || (want_data && !d->w) || ((want_data || d->gw) && (!d->x || !d->offmask))) return YMI_ENULL;
  if (((uintptr_t)d->x | (uintptr_t)d->gy | (uintptr_t)d->gx) & 15) return YMI_ESHAPE;

  hipStream_t s = (hipStream_t)stream;
  int rc = YMI_OK;
  BwdParams p;
  p.x = d->x; p.offmask = d->offmask; p.w = d->w; p.gy = d->gy;
  p.gx = d->gx; p.goff = d->g_offset; p.gmask = d->g_mask; p.gw = d->gw; p.gbias = d->gbias;
  p.B = d->B; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.ldx = d->ldx; p.Ho = d->Ho; p.Wo = d->Wo; p.Cout = d->Cout;
  p.stride = d->stride; p.ldo = d->ldo; p.om_layout = d->om_layout;
  p.M = (int)M; p.HoWo = d->Ho * d->Wo;
  p.ncc = d->Cin / 32; p.cc_per_blk = p.ncc; p.atomic_om = 0; p.m_per_blk = 32;

  if (want_data) {
    const int bm = (int)((M + 31) / 32);
    // small maps: spread the channel chunks over blocks (at least four per block, one per wave) until ~512 blocks exist
    int cs = 1;
    while (bm * cs < 512 && p.ncc / (2 * cs) >= 4) cs *= 2;
    p.cc_per_blk = (p.ncc + cs - 1) / cs;
    cs = (p.ncc + p.cc_per_blk - 1) / p.cc_per_blk;
    p.atomic_om = cs > 1;
    if (d->gx && hipMemsetAsync(d->gx, 0, (size_t)d->B * d->H * d->W * d->ldx * sizeof(float), s) != hipSuccess) return ymi_launch_status();
    if (p.atomic_om) {
      if (d->g_offset && hipMemsetAsync(d->g_offset, 0, (size_t)M * 18 * sizeof(float), s) != hipSuccess) return ymi_launch_status();
      if (d->g_mask && hipMemsetAsync(d->g_mask, 0, (size_t)M * 9 * sizeof(float), s) != hipSuccess) return ymi_launch_status();
    }
    rc = ymi_launch(dcn_bwd_data_k, dim3(bm, cs), dim3(256), 0, stream, p);
  }
  if (!rc && want_w) {
    if (d->gw && hipMemsetAsync(d->gw, 0, (size_t)d->Cout * 9 * d->Cin * sizeof(float), s) != hipSuccess) return ymi_launch_status();
    if (d->gbias && hipMemsetAsync(d->gbias, 0, (size_t)d->Cout * sizeof(float), s) != hipSuccess) return ymi_launch_status();
    const int gx_ = d->gw ? 9 * p.ncc : 1;              // bias alone: the blocks of tap 0, channels 0 .. 31
    const ymi_wgrad_tiles t = ymi_wgrad_nt(d->Cout);
    const ymi_chunks c = ymi_chunk_plan(M, 1024, (long)gx_ * t.gz);       // ranges of m
    p.m_per_blk = (int)c.per;
    void (*const kernels[3])(BwdParams) = {dcn_bwd_weight_k<1>, dcn_bwd_weight_k<2>, dcn_bwd_weight_k<4>};
    rc = ymi_launch(kernels[t.nt >> 1], dim3(gx_, c.nchunks, t.gz), dim3(256), 0, stream, p);      // nt = 1, 2, 4
  }
  return rc;
}
