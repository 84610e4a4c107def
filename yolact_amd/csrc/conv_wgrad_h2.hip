// ymi_conv_wgrad_nhwc_h2: the weight gradient of ymi_conv_wgrad_nhwc_f32 (conv_train.hip) on the fp16 matrix pipe, opt-in
// (train_ops.wgrad_mode('fp16x2')).  dw[k,co] = sum_pos im2col(x)[pos,k] g[pos,co] with BOTH operands carried as two fp16 planes
// under one power-of-two scale per tensor (gemm_h2.h: t = v s, h = fp16(t), l = fp16(t - h)); every product is hh + hl + lh on
// v_mfma_f32_32x32x16_f16 with fp32 accumulation.  db[co] = sum_pos g[pos,co] stays plain fp32.  No floating-point atomics: the order
// of additions is a function of the shape only.
//
// Three launches:
//   wgrad_h2_prep_k   (a) two offset tables, so that the main kernel does no coordinate arithmetic: xoff[tap][pos] = the byte offset
//                     in x of the pixel tap (ky, kx) of position pos = (n, oy, ox) reads, gofs[pos] = the byte offset of g's row pos;
//                     a pixel outside the map and a position >= P hold OOB (gemm_h2.h), which a buffer load answers with 0.0.
//                     (b) the magnitude bounds: max |x| over all of x and max |g| over the channels [0, Cout), as integer maxima of
//                     the bit patterns with the sign cleared (order-free, no floating-point atomics, a NaN counts as above Inf): one
//                     partial per block to ws, NB of them per tensor.  Every later wave takes the maximum of the NB partials itself.
//   wgrad_h2_k<NT>    the blocking of wgrad_k: a block owns one (tap, 32 input channels), one chunk of positions and NT * 128 output
//                     channels, each wave NT column tiles of 32.  NT is 1 for Cout <= 128 and 2 above it (h2_plan): with four tiles a
//                     wave needs the SIMD to itself, and then nothing overlaps its splits (VALU) with its MFMAs; two waves per SIMD
//                     do.  The chunks are ymi_chunk_plan(P, 1024, taps * (Cin / 32) * ceil(Cout / (NT * 128))): the fp32 entry's rule,
//                     and its very chunks up to Cout = 256.  The
//                     positions are the instruction's k index: a K-step is 16 positions, lane (ln, kk) holds positions 8 kk .. 8 kk + 7
//                     of channel ln, read by eight 4-byte buffer loads (32 lanes = 128 contiguous bytes).  Per K-step the x fragment
//                     is split once and feeds the wave's NT tiles; per tile j, in this order over the tiles,
//                         acc[j] += xh gh,   then   acc[j] += xh gl,   then   acc[j] += xl gh.
//                     The loads of a K-step are issued one K-step ahead of the MFMAs that use them, the table rows two further ahead.
//                     db: a lane adds its 8 positions of every K-step in ascending order, then half 0 + half 1.
//   wgrad_h2_sum_k    the chunk partials in chunk order from +0.0 (ymi_chunk_sum), then the scales undone by TWO multiplications with
//                     2^(e >> 1) and 2^(e - (e >> 1)), e = the sum of the two inverse scales' exponents: s_x s_g is never formed as
//                     a float, and both factors move the value the same way, so nothing overflows or underflows that the result does
//                     not.  A bound of 0: s = 1, every product is +-0, acc stays +0.0 and dw = +0.0.
#include "wgrad_plan.h"
#include "gemm_h2.h"

namespace {
using namespace ymi_h2;

constexpr int NB = 1024;       // blocks of the first launch = partial maxima per tensor (a multiple of 64)
constexpr int SLACK = 64;      // table entries past the last chunk that the main kernel's read-ahead may touch

struct HwParams {
  const float *x, *g;
  float *dw, *db, *ws_w, *ws_b;
  unsigned *xoff, *gofs, *amax;                        // [taps][Ppad] + SLACK, [Ppad] + SLACK, [2][NB]
  int H, W, Cin, Cout, ldg, kw, pad, S, ncc, gx, K, taps, nchunks, want_w, want_b, Ho, Wo;
  long P, per, Ppad, nx;                               // nx: elements of x
  int xbytes, gbytes;
  int vec;                                             // x and g 16-byte aligned, ldg % 4 == 0: the bounds read 16 bytes per load
};

// the maximum of the NB partial bounds at a, the same value in every lane (every lane of the wave must call it)
__device__ __forceinline__ float h2_bound(const unsigned *a) {
  const int lane = threadIdx.x & 63;
  unsigned v = 0;
#pragma unroll
  for (int i = 0; i < NB / 64; ++i) { const unsigned u = a[lane + 64 * i]; v = u > v ? u : v; }
  v = ymi_wave_umax63(v);
  return __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_readlane((int)v, 63));
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void wgrad_h2_prep_k(const HwParams p) {
  __shared__ unsigned red[2][4];
  const long t0 = (long)blockIdx.x * 256 + threadIdx.x, nthr = (long)NB * 256;
  const long nxo = (long)p.taps * p.Ppad + SLACK, ngo = p.Ppad + SLACK;
  for (long i = t0; i < nxo + ngo; i += nthr) {
    unsigned off = OOB;
    if (i < nxo) {
      const long tap = i / p.Ppad, pos = i - tap * p.Ppad;
      if (tap < p.taps && pos < p.P) {
        const int ox = (int)(pos % p.Wo);
        const long r = pos / p.Wo;
        const int oy = (int)(r % p.Ho), n = (int)(r / p.Ho);
        const int ky = (int)tap / p.kw, kx = (int)tap - ky * p.kw;
        const int iy = p.S * oy + ky - p.pad, ix = p.S * ox + kx - p.pad;
        if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
          off = (unsigned)(4 * ((((long)n * p.H + iy) * p.W + ix) * p.Cin));     // < 2^31 (validate_wgrad)
      }
      p.xoff[i] = off;
    } else {
      const long pos = i - nxo;
      if (pos < p.P) off = (unsigned)(4 * pos * p.ldg);
      p.gofs[pos] = off;
    }
  }
  unsigned mx = 0, mg = 0;
  if (p.want_w) {
    const unsigned *xb = reinterpret_cast<const unsigned *>(p.x), *gb = reinterpret_cast<const unsigned *>(p.g);
    const unsigned nx = (unsigned)p.nx, ng = (unsigned)(p.P * p.ldg), ldg = (unsigned)p.ldg, Cout = (unsigned)p.Cout;   // < 2^29 each
    if (p.vec) {                                       // (Cin % 32 == 0: nx is a multiple of 4; a group of 4 stays inside a row of g)
      const u32x4 *x4 = reinterpret_cast<const u32x4 *>(p.x), *g4 = reinterpret_cast<const u32x4 *>(p.g);
      for (unsigned i = (unsigned)t0; i < nx / 4; i += NB * 256) {
        const u32x4 v = x4[i] & 0x7fffffffu;
        const unsigned a = v[0] > v[1] ? v[0] : v[1], b = v[2] > v[3] ? v[2] : v[3], c = a > b ? a : b;
        mx = c > mx ? c : mx;
      }
      for (unsigned i = (unsigned)t0; i < ng / 4; i += NB * 256) {
        const u32x4 v = g4[i] & 0x7fffffffu;
        const unsigned c = (4u * i) % ldg;
#pragma unroll
        for (int e = 0; e < 4; ++e) mg = (c + e < Cout && v[e] > mg) ? v[e] : mg;
      }
    } else {
      for (unsigned i = (unsigned)t0; i < nx; i += NB * 256) { const unsigned u = xb[i] & 0x7fffffffu; mx = u > mx ? u : mx; }
      for (unsigned i = (unsigned)t0; i < ng; i += NB * 256) {
        if (i % ldg < Cout) { const unsigned u = gb[i] & 0x7fffffffu; mg = u > mg ? u : mg; }
      }
    }
  }
  mx = ymi_wave_umax63(mx); mg = ymi_wave_umax63(mg);
  if ((threadIdx.x & 63) == 63) { red[0][threadIdx.x >> 6] = mx; red[1][threadIdx.x >> 6] = mg; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const unsigned *r = red[threadIdx.x];
    const unsigned a = r[0] > r[1] ? r[0] : r[1], b = r[2] > r[3] ? r[2] : r[3];
    p.amax[threadIdx.x * NB + blockIdx.x] = a > b ? a : b;
  }
}

// NT: 32-column output-channel tiles per wave (a block covers NT * 128 output channels)
template <int NT> __global__ __launch_bounds__(256, 2) void wgrad_h2_k(const HwParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ln = lane & 31, kk = lane >> 5;
  // blockIdx.x = (group of NT * 128 output channels, tap, 32 input channels): no 65535 limit on the groups
  const int bx = (int)(blockIdx.x % (unsigned)p.gx);
  const int tap = bx / p.ncc, c0 = (bx % p.ncc) * 32;
  const int ob = (int)(blockIdx.x / (unsigned)p.gx) * (NT * 128);
  const long pos0 = (long)blockIdx.y * p.per;
  const long pos1 = pos0 + p.per < p.P ? pos0 + p.per : p.P;
  const bool do_w = p.want_w != 0;
  const bool do_bias = p.want_b != 0 && bx == 0;

  // the wave's column tiles that hold a real output channel are a prefix of its NT tiles
  int nact = 0;
#pragma unroll
  for (int j = 0; j < NT; ++j) nact += (ob + (wave + 4 * j) * 32 < p.Cout) ? 1 : 0;
  if (nact == 0) return;                               // (no barrier below)

  float sx, sg, inv;
  ymi_h2_scale(h2_bound(p.amax), sx, inv);
  ymi_h2_scale(h2_bound(p.amax + NB), sg, inv);

  f32x16 acc[NT];
  float bs[NT];
  bool col[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    bs[j] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    col[j] = ob + (wave + 4 * j) * 32 + ln < p.Cout;
  }

  // every read of x and g is a range-checked buffer load: OOB table entries, rows past g and (without dw) all of x answer 0.0
  const __amdgpu_buffer_rsrc_t xrs = buf_rsrc(p.x, do_w ? p.xbytes : 0), grs = buf_rsrc(p.g, p.gbytes);
  const unsigned xlane = 4u * (unsigned)(c0 + ln), glane = 4u * (unsigned)(ob + wave * 32 + ln);
  const unsigned *xt = p.xoff + (size_t)tap * p.Ppad + pos0 + 8 * kk, *gt = p.gofs + pos0 + 8 * kk;

  struct Tab { u32x4 x0, x1, g0, g1; };                // this lane's 8 positions of one K-step: the offsets in x and in g
  struct Raw { float a[8]; float b[NT][8]; };
  auto table = [&](Tab &T, int q) {                    // (16-byte aligned: Ppad, pos0, 8 kk and 16 q are multiples of 4 entries)
    T.x0 = *reinterpret_cast<const u32x4 *>(xt + 16 * q); T.x1 = *reinterpret_cast<const u32x4 *>(xt + 16 * q + 4);
    T.g0 = *reinterpret_cast<const u32x4 *>(gt + 16 * q); T.g1 = *reinterpret_cast<const u32x4 *>(gt + 16 * q + 4);
  };
  auto issue = [&](Raw &R, const Tab &T) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned xo = (e < 4 ? T.x0[e & 3] : T.x1[e & 3]) + xlane, go = (e < 4 ? T.g0[e & 3] : T.g1[e & 3]) + glane;
      R.a[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, xo, 0, 0));
#pragma unroll
      for (int j = 0; j < NT; ++j)
        R.b[j][e] = j < nact ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(grs, go + 512u * j, 0, 0)) : 0.f;
    }
  };
  auto consume = [&](const Raw &R) {
    Frag fa, fb[NT];
    if (do_w) fa = split8h(f32x4{R.a[0], R.a[1], R.a[2], R.a[3]}, f32x4{R.a[4], R.a[5], R.a[6], R.a[7]}, sx);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      if (j < nact) {
        float b[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { b[e] = col[j] ? R.b[j][e] : 0.f; bs[j] += b[e]; }
        if (do_w) fb[j] = split8h(f32x4{b[0], b[1], b[2], b[3]}, f32x4{b[4], b[5], b[6], b[7]}, sg);
      }
    }
    if (do_w) {
#pragma unroll
      for (int j = 0; j < NT; ++j) if (j < nact) acc[j] = ymi_mfma32(fa.h, fb[j].h, acc[j]);
#pragma unroll
      for (int j = 0; j < NT; ++j) if (j < nact) acc[j] = ymi_mfma32(fa.h, fb[j].l, acc[j]);
#pragma unroll
      for (int j = 0; j < NT; ++j) if (j < nact) acc[j] = ymi_mfma32(fa.l, fb[j].h, acc[j]);
    }
  };

  // K-steps of the chunk, an even count (a chunk is a multiple of 32 positions; past P everything reads 0.0).  The read-ahead
  // touches table rows of up to 3 K-steps past the chunk: the next chunk's, the next tap's or the SLACK entries.
  const int nq = (int)((pos1 - pos0 + 31) / 32) * 2;
  Tab T0, T1;
  Raw R0, R1;
  table(T0, 0); table(T1, 1);
  issue(R0, T0); table(T0, 2);
  for (int q = 0; q < nq; q += 2) {
    issue(R1, T1); table(T1, q + 3);
    consume(R0);
    issue(R0, T0); table(T0, q + 4);
    consume(R1);
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
      const float v = bs[j] + __shfl_xor(bs[j], 32);   // positions 0 .. 7 of every K-step + positions 8 .. 15
      const int o = ob + (wave + 4 * j) * 32 + ln;
      if (j < nact && kk == 0 && o < p.Cout) p.ws_b[(size_t)blockIdx.y * p.Cout + o] = v;
    }
  }
#endif
}

// thread = one element of dw [K, Cout], then of db [Cout]
__global__ __launch_bounds__(256) void wgrad_h2_sum_k(const HwParams p) {
  float s, ix, ig;
  ymi_h2_scale(h2_bound(p.amax), s, ix);
  ymi_h2_scale(h2_bound(p.amax + NB), s, ig);
  const long i = (long)blockIdx.x * 256 + threadIdx.x, nw = (long)p.K * p.Cout;
  if (i < nw) {
    if (!p.want_w) return;
    // 1 / (s_x s_g) = 2^e as two factors of the same direction
    const int e = (int)(__builtin_bit_cast(unsigned, ix) >> 23) + (int)(__builtin_bit_cast(unsigned, ig) >> 23) - 254;
    const int e1 = e >> 1, e2 = e - e1;
    const float m1 = __builtin_bit_cast(float, (unsigned)(e1 + 127) << 23), m2 = __builtin_bit_cast(float, (unsigned)(e2 + 127) << 23);
    p.dw[i] = (ymi_chunk_sum(p.ws_w, nw, p.nchunks, i) * m1) * m2;
  } else if (i < nw + p.Cout) {
    if (!p.want_b) return;
    const int o = (int)(i - nw);
    p.db[o] = ymi_chunk_sum(p.ws_b, p.Cout, p.nchunks, o);
  }
}

// the decomposition for a validated shape: wgrad_plan's with at most two column tiles per wave
WgPlan h2_plan(const ymi_conv_wgrad_desc *d) {
  const int nt = d->Cout <= 128 ? 1 : 2, gz = (d->Cout + nt * 128 - 1) / (nt * 128);
  const int gx = d->kh * d->kw * (d->Cin / 32);
  const ymi_chunks c = ymi_chunk_plan(wgrad_positions(d), 1024, (long)gx * gz);
  return {nt, gx, gz, c.nchunks, c.per};
}

struct HwLayout { int64_t off[5], total; };

// Workspace: [nchunks][kh*kw*Cin][Cout] floats, [nchunks][Cout] floats, the two offset tables, the partial bounds
HwLayout h2_layout(const ymi_conv_wgrad_desc *d, const WgPlan &w) {
  const int64_t K = (int64_t)d->kh * d->kw * d->Cin, Ppad = (int64_t)w.nchunks * w.per;
  const int64_t sizes[5] = {(int64_t)w.nchunks * K * d->Cout, (int64_t)w.nchunks * d->Cout, (int64_t)d->kh * d->kw * Ppad + SLACK, Ppad + SLACK,
                            2 * NB};
  HwLayout l;
  l.total = ymi_ws_layout(sizes, l.off);
  return l;
}

}  // namespace

extern "C" int64_t ymi_conv_wgrad_h2_ws_bytes(const ymi_conv_wgrad_desc *d) {
  const int rc = validate_wgrad(d);
  if (rc) return rc;
  if (wgrad_plan(d).gz > 65535) return YMI_ESHAPE;            // (the fp32 entry's limit: the two reject the same descriptors)
  return h2_layout(d, h2_plan(d)).total;
}

extern "C" int ymi_conv_wgrad_nhwc_h2(const ymi_conv_wgrad_desc *d, void *stream) {
  const int rc = validate_wgrad(d);
  if (rc) return rc;
  if (!d->g || (!d->dw && !d->db) || (d->dw && !d->x) || !d->ws) return YMI_ENULL;
  if ((uintptr_t)d->ws & 15) return YMI_ESHAPE;
  if (wgrad_plan(d).gz > 65535) return YMI_ESHAPE;
  const WgPlan w = h2_plan(d);
  const HwLayout l = h2_layout(d, w);
  if (d->ws_bytes < l.total) return YMI_ESHAPE;
  char *ws = static_cast<char *>(d->ws);
  HwParams p;
  p.x = d->x; p.g = d->g; p.dw = d->dw; p.db = d->db;
  p.ws_w = reinterpret_cast<float *>(ws + l.off[0]); p.ws_b = reinterpret_cast<float *>(ws + l.off[1]);
  p.xoff = reinterpret_cast<unsigned *>(ws + l.off[2]); p.gofs = reinterpret_cast<unsigned *>(ws + l.off[3]);
  p.amax = reinterpret_cast<unsigned *>(ws + l.off[4]);
  p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.Cout = d->Cout; p.ldg = d->ldg; p.kw = d->kw; p.pad = d->pad; p.S = d->stride == 2 ? 2 : 1;
  p.ncc = d->Cin / 32; p.K = d->kh * d->kw * d->Cin; p.taps = d->kh * d->kw; p.nchunks = w.nchunks;
  p.want_w = d->dw != nullptr; p.want_b = d->db != nullptr;
  p.Ho = wgrad_out(d, d->H, d->kh); p.Wo = wgrad_out(d, d->W, d->kw);
  p.P = wgrad_positions(d); p.per = w.per; p.Ppad = (long)w.nchunks * w.per; p.nx = (long)d->B * d->H * d->W * d->Cin;
  p.vec = (((uintptr_t)d->x | (uintptr_t)d->g) & 15) == 0 && d->ldg % 4 == 0;
  p.xbytes = (int)(4 * p.nx); p.gbytes = (int)(4 * p.P * d->ldg);     // < 2^31 (validate_wgrad)
  p.gx = d->dw ? w.gx : 1;                                   // bias alone: the blocks of tap 0, channels 0 .. 31
  const dim3 grid((unsigned)p.gx * w.gz, w.nchunks);
  int rl = ymi_launch(wgrad_h2_prep_k, dim3(NB), dim3(256), 0, stream, p);
  if (!rl) rl = ymi_launch(w.nt == 1 ? wgrad_h2_k<1> : wgrad_h2_k<2>, grid, dim3(256), 0, stream, p);
  if (!rl) rl = ymi_launch(wgrad_h2_sum_k, dim3((unsigned)(((long)p.K * d->Cout + d->Cout + 255) / 256)), dim3(256), 0, stream, p);
  return rl;
}
