// JPEG encoding on the GPU: eval.py's cv2.imwrite(save_path, img_numpy) for a frame that is already on the device
// (display.prep_display).  Input uint8 BGR [h,w,3]; output the entropy-coded scan + EOI, byte-equal to libjpeg-turbo's.
//   jpeg_enc_dct_k      per 8x8 block of the scan (8 threads each): BGR -> Y / Cb / Cr, edge replication, h2v2 downsampling,
//                       ISLOW forward DCT (row pass in registers, column pass through LDS), quantisation -> int16, zigzag order
//   jpeg_enc_count_k    one thread per block: coded bit count (DC difference against the previous block of the component),
//                       exclusive scan inside the group of 256, the group's total
//   jpeg_enc_scan_k     one workgroup: exclusive scan of the per-group totals (uint32 -> uint64) and the grand total
//   jpeg_enc_bits_k     one thread per block: its code bits at its bit offset; whole words are stored, the two words it may share
//                       with its neighbours are combined with atomicOr (the buffer is zeroed first)
//   jpeg_enc_ffcount_k  0xFF bytes per 4096-byte chunk of the unstuffed scan (final byte padded with 1-bits)
//   jpeg_enc_scan_k     again, over the chunks
//   jpeg_enc_stuff_k    scatter: every 0xFF followed by 0x00; the thread that owns the last byte appends EOI and writes the length
// One memset and seven launches on the caller's stream; no host synchronisation, no allocation, no inter-workgroup waiting.
// The arithmetic and the code tables live in jpeg_enc_math.h (shared with the header writer and the g++-built host emulation).
// Byte / integer work on 0.9 MB per 550 x 550 frame: launch-latency bound, not bandwidth bound.
#include "common.h"
#include "../../include/yolact_amd.h"
#include "jpeg_enc_math.h"

extern "C" int64_t ymi_jpeg_enc_layout(int h, int w, int sub, int64_t off[8], int64_t *out_bound);   // jpeg_enc_host.cpp

namespace {

using namespace ymi_jpeg_enc;

__global__ __launch_bounds__(256) void jpeg_enc_dct_k(const uint8_t *__restrict__ img, int64_t stride, const Geom g, int quality,
                                                      int16_t *__restrict__ coef) {
  __shared__ int s_ws[32][8][9];      // [block][row][col], padded
  __shared__ __attribute__((aligned(16))) int16_t s_zz[32][64];
  __shared__ uint16_t s_q[2][64];
  const int tid = threadIdx.x, lb = tid >> 3, t = tid & 7;
  if (tid < 128) s_q[tid >> 6][tid & 63] = (uint16_t)quant_value(quality, tid >> 6, tid & 63);
  const int64_t sb = (int64_t)blockIdx.x * 32 + lb;
  const bool live = sb < g.nblk;
  BlockPos p;
  if (live) {   // pass 1: row t
    p = block_of(g, sb);
    long d[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) d[c] = block_sample(g, p, img, stride, t, c);
    fdct8(d, true);
#pragma unroll
    for (int c = 0; c < 8; ++c) s_ws[lb][t][c] = (int)d[c];
  }
  __syncthreads();
  if (live) {   // pass 2: column t
    long d[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = s_ws[lb][r][t];
    fdct8(d, false);
    const int tq = p.comp ? 1 : 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int n = r * 8 + t;
      const int v = quantize(d[r], s_q[tq][n]);
      s_zz[lb][zigzag_inv(n)] = (int16_t)((p.dummy && n) ? 0 : v);
    }
  }
  __syncthreads();
  if (live) *reinterpret_cast<uint4 *>(coef + sb * 64 + t * 8) = *reinterpret_cast<const uint4 *>(&s_zz[lb][t * 8]);
}

// the four code tables into LDS: tab [4][256], (code << 5) | length
__device__ __forceinline__ void load_tables(uint32_t *s_tab) {
  huff_fill(s_tab, threadIdx.x, 256);
  __syncthreads();
  for (int i = threadIdx.x; i < 12 + 12 + 162 + 162; i += 256) {
    const int tbl = i < 12 ? 0 : (i < 24 ? 1 : (i < 186 ? 2 : 3));
    huff_put(s_tab, tbl, i - (tbl == 0 ? 0 : (tbl == 1 ? 12 : (tbl == 2 ? 24 : 186))));
  }
  __syncthreads();
}

// exclusive scan of one uint32 per thread over a workgroup of NW waves; total = the sum.  s_w: NW + 1 words of LDS.
template <int NW>
__device__ __forceinline__ uint32_t wg_excl_scan(uint32_t v, uint32_t *s_w, uint32_t &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  __syncthreads();      // s_w may still be read from a previous call
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  uint32_t base = 0, sum = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const uint32_t x = s_w[i];
    if (i < wave) base += x;
    sum += x;
  }
  total = sum;
  return base + inc - v;
}

__device__ __forceinline__ void load_block(const int16_t *coef, int64_t sb, uint32_t pk[32]) {
  const uint4 *src = reinterpret_cast<const uint4 *>(coef + sb * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint4 v = src[i];
    pk[4 * i] = v.x; pk[4 * i + 1] = v.y; pk[4 * i + 2] = v.z; pk[4 * i + 3] = v.w;
  }
}

__global__ __launch_bounds__(256) void jpeg_enc_count_k(const int16_t *__restrict__ coef, const Geom g,
                                                        uint32_t *__restrict__ blk_off, uint32_t *__restrict__ grp_bits) {
  __shared__ uint32_t s_tab[4 * 256];
  __shared__ uint32_t s_w[4];
  load_tables(s_tab);
  const int64_t sb = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t bits = 0;
  if (sb < g.nblk) {
    const BlockPos p = block_of(g, sb);
    uint32_t pk[32];
    load_block(coef, sb, pk);
    const int pred = p.prev >= 0 ? (int)coef[p.prev * 64] : 0;
    CountSink c{0};
    encode_block(pk, pred, s_tab + (p.comp ? 256 : 0), s_tab + (p.comp ? 768 : 512), c);
    bits = c.n;
  }
  uint32_t total;
  const uint32_t excl = wg_excl_scan<4>(bits, s_w, total);
  if (sb < g.nblk) blk_off[sb] = excl;
  if (threadIdx.x == 0) grp_bits[blockIdx.x] = total;
}

// one workgroup of 1024: out[i] = sum in[0 .. i), *total = sum in[0 .. n).  A tile of 1024 inputs sums to < 2^32 for both
// uses (<= 256 * 1660 bits per group, <= 4096 bytes per chunk).
__global__ __launch_bounds__(1024) void jpeg_enc_scan_k(const uint32_t *__restrict__ in, uint64_t *__restrict__ out, int64_t n,
                                                        uint64_t *__restrict__ total) {
  __shared__ uint32_t s_w[16];
  uint64_t carry = 0;
  for (int64_t base = 0; base < n; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const uint32_t v = i < n ? in[i] : 0;
    uint32_t tile;
    const uint32_t excl = wg_excl_scan<16>(v, s_w, tile);
    if (i < n) out[i] = carry + excl;
    carry += tile;
  }
  if (threadIdx.x == 0) *total = carry;
}

// MSB-first bit writer into 32-bit words kept in stream byte order.  The first word written and the final partial word can hold
// bits of the neighbouring blocks: atomicOr; every word between is owned by this block alone: plain store.
struct WordSink {
  uint32_t *w;
  uint64_t acc;
  int cnt;
  bool first;
  __device__ __forceinline__ void put(uint32_t code, int nbits) {
    acc = (acc << nbits) | code;
    cnt += nbits;
    if (cnt >= 32) {
      const uint32_t v = __builtin_bswap32((uint32_t)(acc >> (cnt - 32)));
      cnt -= 32;
      acc &= (1ull << cnt) - 1;
      if (first) { atomicOr(w, v); first = false; } else { *w = v; }
      ++w;
    }
  }
  __device__ __forceinline__ void finish() {
    if (cnt) atomicOr(w, __builtin_bswap32((uint32_t)(acc << (32 - cnt))));
  }
};

__global__ __launch_bounds__(256) void jpeg_enc_bits_k(const int16_t *__restrict__ coef, const Geom g,
                                                       const uint32_t *__restrict__ blk_off, const uint64_t *__restrict__ grp_off,
                                                       uint32_t *__restrict__ raw) {
  __shared__ uint32_t s_tab[4 * 256];
  load_tables(s_tab);
  const int64_t sb = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (sb >= g.nblk) return;
  const BlockPos p = block_of(g, sb);
  uint32_t pk[32];
  load_block(coef, sb, pk);
  const int pred = p.prev >= 0 ? (int)coef[p.prev * 64] : 0;
  const uint64_t off = grp_off[blockIdx.x] + blk_off[sb];
  WordSink s{raw + (off >> 5), 0, (int)(off & 31), true};
  encode_block(pk, pred, s_tab + (p.comp ? 256 : 0), s_tab + (p.comp ? 768 : 512), s);
  s.finish();
}

// 16 bytes of the unstuffed scan at byte `base`; the scan is T bytes, the last of them padded with 1-bits (raw is zero beyond)
__device__ __forceinline__ uint4 load_raw16(const uint32_t *raw, int64_t base, uint64_t bits, int64_t T) {
  uint4 v = *reinterpret_cast<const uint4 *>(raw + (base >> 2));
  const int64_t last = T - 1;
  if (last >= base && last < base + 16 && (bits & 7)) {
    const uint32_t pad = ((1u << (8 - (int)(bits & 7))) - 1) << (8 * (int)(last & 3));
    const int wi = (int)((last - base) >> 2);
    if (wi == 0) v.x |= pad; else if (wi == 1) v.y |= pad; else if (wi == 2) v.z |= pad; else v.w |= pad;
  }
  return v;
}
__device__ __forceinline__ uint32_t count_ff(uint32_t w) {
  return ((w & 0xFF) == 0xFF) + ((w & 0xFF00) == 0xFF00) + ((w & 0xFF0000) == 0xFF0000) + ((w >> 24) == 0xFF);
}

__global__ __launch_bounds__(256) void jpeg_enc_ffcount_k(const uint32_t *__restrict__ raw, const uint64_t *__restrict__ totals,
                                                          uint32_t *__restrict__ ff_cnt) {
  __shared__ uint32_t s_w[4];
  const uint64_t bits = totals[0];
  const int64_t T = (int64_t)((bits + 7) >> 3);
  const int64_t base = (int64_t)blockIdx.x * 4096 + threadIdx.x * 16;
  uint32_t n = 0;
  if (base < T) {
    const uint4 v = load_raw16(raw, base, bits, T);
    n = count_ff(v.x) + count_ff(v.y) + count_ff(v.z) + count_ff(v.w);
  }
  uint32_t total;
  wg_excl_scan<4>(n, s_w, total);
  if (threadIdx.x == 0) ff_cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void jpeg_enc_stuff_k(const uint32_t *__restrict__ raw, const uint64_t *__restrict__ totals,
                                                        const uint64_t *__restrict__ ff_off, uint8_t *__restrict__ out,
                                                        int64_t *__restrict__ out_len) {
  __shared__ uint32_t s_w[4];
  const uint64_t bits = totals[0];
  const int64_t T = (int64_t)((bits + 7) >> 3);
  if ((int64_t)blockIdx.x * 4096 >= T) return;      // uniform over the workgroup
  const int64_t base = (int64_t)blockIdx.x * 4096 + threadIdx.x * 16;
  uint4 v = make_uint4(0, 0, 0, 0);
  uint32_t n = 0;
  if (base < T) {
    v = load_raw16(raw, base, bits, T);
    n = count_ff(v.x) + count_ff(v.y) + count_ff(v.z) + count_ff(v.w);
  }
  uint32_t total;
  const uint32_t excl = wg_excl_scan<4>(n, s_w, total);
  if (base >= T) return;
  uint8_t *o = out + base + (int64_t)ff_off[blockIdx.x] + excl;
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (base + i < T) {
      const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xFF;
      *o++ = (uint8_t)b;
      if (b == 0xFF) *o++ = 0;
    }
  }
  if (T - 1 < base + 16) {      // this thread wrote the last byte of the scan
    o[0] = 0xFF; o[1] = 0xD9;
    *out_len = (int64_t)(o - out) + 2;
  }
}

}  // namespace

extern "C" int ymi_jpeg_encode_bgr_u8(const ymi_jpeg_enc_desc *d, void *stream) {
  if (!d) return YMI_ENULL;
  if (!d->img || !d->out || !d->out_len || !d->ws) return YMI_ENULL;
  if (d->quality < 1 || d->quality > 100) return YMI_EARG;
  int64_t off[8], bound = 0;
  const int64_t total = ymi_jpeg_enc_layout(d->h, d->w, d->subsampling, off, &bound);
  if (total < 0) return YMI_EARG;
  if (d->row_stride < 3 * (int64_t)d->w || d->out_capacity < bound) return YMI_EARG;
  if ((uintptr_t)d->ws & 255) return YMI_ESHAPE;
  hipStream_t s = (hipStream_t)stream;
  const Geom g = make_geom(d->h, d->w, d->subsampling);
  uint8_t *ws = (uint8_t *)d->ws;
  int16_t *coef = (int16_t *)(ws + off[0]);
  uint32_t *blk_off = (uint32_t *)(ws + off[1]), *grp_bits = (uint32_t *)(ws + off[2]);
  uint64_t *grp_off = (uint64_t *)(ws + off[3]), *totals = (uint64_t *)(ws + off[4]);
  uint32_t *raw = (uint32_t *)(ws + off[5]), *ff_cnt = (uint32_t *)(ws + off[6]);
  uint64_t *ff_off = (uint64_t *)(ws + off[7]);
  const int64_t raw_bytes = off[6] - off[5];
  const int64_t ngrp = (g.nblk + 255) / 256, nchunk = (g.nblk * MAX_BLOCK_BYTES + 4095) / 4096;
  const hipError_t e = hipMemsetAsync(raw, 0, (size_t)raw_bytes, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(jpeg_enc_dct_k, dim3((unsigned)((g.nblk + 31) / 32)), dim3(256), 0, s, d->img, d->row_stride, g, d->quality,
                     coef);
  hipLaunchKernelGGL(jpeg_enc_count_k, dim3((unsigned)ngrp), dim3(256), 0, s, coef, g, blk_off, grp_bits);
  hipLaunchKernelGGL(jpeg_enc_scan_k, dim3(1), dim3(1024), 0, s, grp_bits, grp_off, ngrp, totals);
  hipLaunchKernelGGL(jpeg_enc_bits_k, dim3((unsigned)ngrp), dim3(256), 0, s, coef, g, blk_off, grp_off, raw);
  hipLaunchKernelGGL(jpeg_enc_ffcount_k, dim3((unsigned)nchunk), dim3(256), 0, s, raw, totals, ff_cnt);
  hipLaunchKernelGGL(jpeg_enc_scan_k, dim3(1), dim3(1024), 0, s, ff_cnt, ff_off, nchunk, totals + 1);
  hipLaunchKernelGGL(jpeg_enc_stuff_k, dim3((unsigned)nchunk), dim3(256), 0, s, raw, totals, ff_off, d->out, d->out_len);
  return ymi_launch_status();
}
