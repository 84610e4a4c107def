// Arithmetic of the JPEG encoder kernels (jpeg_enc.hip), shared verbatim with the header writer (jpeg_enc_host.cpp) and with
// the host emulation that the CPU tests build with g++ (tests/jpeg_enc_emul.cpp): the SAME inline functions run per block on
// both sides, so the integer arithmetic and the code tables are checked against libjpeg-turbo (through Pillow) without a GPU and
// the GPU test only has to prove the launch geometry.  No HIP types here.
//   quant_value                 jcparam.c jpeg_set_quality(q, TRUE): T.81 Annex K.1 tables scaled, clamped to 1..255
//   rgb_to_y / _cb / _cr        jccolor.c rgb_ycc_convert (SCALEBITS 16)
//   Geom / block_of / sample    jcprepct.c + jcsample.c edge expansion, h2v2_downsample (bias 1,2,1,2..), jccoefct.c dummy blocks
//   fdct8_pass1 / fdct8_pass2   jfdctint.c jpeg_fdct_islow (CONST_BITS 13, PASS1_BITS 2), rows then columns, output scaled by 8
//   quantize                    jcdctmgr.c: divisor q << 3, round half away from zero
//   huff_entry / encode_block   jchuff.c encode_one_block with the T.81 Annex K.3 tables (jstdhuff.c)
// Corrections against the issue's from-memory list, settled by byte equality with Pillow / libjpeg-turbo:
//   * bottom edge of a SUBSAMPLED component: the image is extended by its last row only to a whole row group (an even row count
//     for 4:2:0); that row group is downsampled, and the rest of the MCU row then repeats the last DOWNSAMPLED row
//     (jcprepct.c pre_process_data).  Extending the image to the whole MCU row first gives other chroma samples when h is even.
#pragma once
#include <stddef.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define YMI_EHD __host__ __device__ __forceinline__
#define YMI_EHM __host__ __device__ __forceinline__      /* member functions */
#else
#define YMI_EHD static inline
#define YMI_EHM inline
#endif

namespace ymi_jpeg_enc {

constexpr int SUB_444 = 0, SUB_420 = 2;      // YMI_JPEG_SUB_* (Pillow's numbering)
constexpr int F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299,
              F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
// worst case of one coded block: DC 11-bit code + 11 magnitude bits, 63 x (16-bit code + 10 magnitude bits) = 1660 bits
constexpr int MAX_BLOCK_BYTES = 208;

YMI_EHD int zigzag(int k) {      // zigzag position -> natural (row-major) index
  const uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return z[k];
}
YMI_EHD int zigzag_inv(int n) {  // natural index -> zigzag position
  const uint8_t z[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                         41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                         46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
  return z[n];
}

// quantisation value of table tbl (0 luminance, 1 chrominance) at natural index n
YMI_EHD int quant_value(int quality, int tbl, int n) {
  const uint8_t base[2][64] = {
      {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
       100, 103, 99},
      {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
       99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int v = ((int)base[tbl][n] * scale + 50) / 100;
  return v < 1 ? 1 : (v > 255 ? 255 : v);
}

YMI_EHD int rgb_to_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
YMI_EHD int rgb_to_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
YMI_EHD int rgb_to_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// Scan geometry.  4:2:0: an MCU is 16x16 pixels = luma blocks (0,0) (1,0) (0,1) (1,1), Cb, Cr; 4:4:4: 8x8 = Y, Cb, Cr.
struct Geom {
  int h, w, sub;
  int mcux, mcuy, bpm;      // MCUs per row / column, blocks per MCU (6 or 3)
  int wib, hib;             // luma size in blocks that hold image samples: ceil(w / 8), ceil(h / 8)
  int64_t nblk;             // blocks in the scan = mcux * mcuy * bpm
};
YMI_EHD Geom make_geom(int h, int w, int sub) {
  Geom g;
  g.h = h; g.w = w; g.sub = sub;
  const int m = sub == SUB_420 ? 16 : 8;
  g.mcux = (w + m - 1) / m; g.mcuy = (h + m - 1) / m; g.bpm = sub == SUB_420 ? 6 : 3;
  g.wib = (w + 7) / 8; g.hib = (h + 7) / 8;
  g.nblk = (int64_t)g.mcux * g.mcuy * g.bpm;
  return g;
}

struct BlockPos {
  int comp;        // 0 Y, 1 Cb, 2 Cr
  int bx, by;      // block coordinates in the component
  int dummy;       // 1: beyond the component's real block grid -> all zero except DC = the DC of block (bx, by)
  int64_t prev;    // scan index of the previous block of the same component (-1: none, predictor 0)
};
// Scan block sb -> where its samples come from.  A dummy block takes the DC of the block BEFORE it in MCU order (jccoefct.c
// compress_data); (bx, by) is then that (real) block, so its DC is recomputed in place and nothing is read across threads.
YMI_EHD BlockPos block_of(const Geom &g, int64_t sb) {
  BlockPos p;
  const int64_t mcu = sb / g.bpm;
  const int k = (int)(sb - mcu * g.bpm);
  const int my = (int)(mcu / g.mcux), mx = (int)(mcu - (int64_t)my * g.mcux);
  p.dummy = 0;
  if (g.sub == SUB_420 && k < 4) {
    p.comp = 0;
    int kk = k;
    while (kk > 0 && (2 * mx + (kk & 1) >= g.wib || 2 * my + (kk >> 1) >= g.hib)) --kk;
    p.dummy = kk != k;
    p.bx = 2 * mx + (kk & 1); p.by = 2 * my + (kk >> 1);
    p.prev = k > 0 ? sb - 1 : (mcu > 0 ? sb - 3 : -1);
  } else {
    p.comp = g.sub == SUB_420 ? k - 3 : k;
    p.bx = mx; p.by = my;
    p.prev = mcu > 0 ? sb - g.bpm : -1;
  }
  return p;
}

YMI_EHD int comp_of_pixel(const uint8_t *px, int comp) {      // px -> B, G, R
  const int b = px[0], g = px[1], r = px[2];
  return comp == 0 ? rgb_to_y(r, g, b) : (comp == 1 ? rgb_to_cb(r, g, b) : rgb_to_cr(r, g, b));
}

// sample (column c, row t) of block p, level-shifted by -128
YMI_EHD int block_sample(const Geom &g, const BlockPos &p, const uint8_t *img, int64_t stride, int t, int c) {
  if (g.sub == SUB_420 && p.comp != 0) {
    const int dh = (g.h + 1) >> 1;
    int j = p.by * 8 + t;
    j = j < dh ? j : dh - 1;
    const int y0 = 2 * j, y1 = 2 * j + 1 < g.h ? 2 * j + 1 : g.h - 1;
    const int i = p.bx * 8 + c;
    const int x0 = 2 * i < g.w ? 2 * i : g.w - 1, x1 = 2 * i + 1 < g.w ? 2 * i + 1 : g.w - 1;
    const uint8_t *r0 = img + (int64_t)y0 * stride, *r1 = img + (int64_t)y1 * stride;
    const int s = comp_of_pixel(r0 + 3 * x0, p.comp) + comp_of_pixel(r0 + 3 * x1, p.comp) + comp_of_pixel(r1 + 3 * x0, p.comp) +
                  comp_of_pixel(r1 + 3 * x1, p.comp);
    return ((s + 1 + (i & 1)) >> 2) - 128;
  }
  int y = p.by * 8 + t, x = p.bx * 8 + c;
  y = y < g.h ? y : g.h - 1;
  x = x < g.w ? x : g.w - 1;
  return comp_of_pixel(img + (int64_t)y * stride + 3 * x, p.comp) - 128;
}

YMI_EHD long fdescale(long x, int n) { return (x + (1L << (n - 1))) >> n; }

// one 1-D pass of jfdctint.c on 8 values, in place; first: the row pass (scales up by PASS1_BITS), else the column pass
YMI_EHD void fdct8(long d[8], bool first) {
  const long tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const long tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  const int sh = first ? 13 - 2 : 13 + 2;
  d[0] = first ? (tmp10 + tmp11) * 4 : fdescale(tmp10 + tmp11, 2);
  d[4] = first ? (tmp10 - tmp11) * 4 : fdescale(tmp10 - tmp11, 2);
  long z1 = (tmp12 + tmp13) * F0_541;
  d[2] = fdescale(z1 + tmp13 * F0_765, sh);
  d[6] = fdescale(z1 + tmp12 * (-(long)F1_847), sh);
  z1 = tmp4 + tmp7;
  long z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const long z5 = (z3 + z4) * F1_175;
  const long t4 = tmp4 * F0_298, t5 = tmp5 * F2_053, t6 = tmp6 * F3_072, t7 = tmp7 * F1_501;
  z1 *= -(long)F0_899; z2 *= -(long)F2_562; z3 *= -(long)F1_961; z4 *= -(long)F0_390;
  z3 += z5; z4 += z5;
  d[7] = fdescale(t4 + z1 + z3, sh);
  d[5] = fdescale(t5 + z2 + z4, sh);
  d[3] = fdescale(t6 + z2 + z3, sh);
  d[1] = fdescale(t7 + z1 + z4, sh);
}

YMI_EHD int quantize(long c, int q) {
  const uint32_t div = (uint32_t)q << 3;      // |c| < 2^16 after the two passes: 32-bit division
  const uint32_t t = (uint32_t)(c < 0 ? -c : c) + (div >> 1);
  const int v = t >= div ? (int)(t / div) : 0;
  return c < 0 ? -v : v;
}

// one whole block: samples -> quantised coefficients in ZIGZAG order (the serial form; the kernel splits the two passes
// over eight threads and calls the same fdct8 / quantize)
YMI_EHD void fdct_quant_block(const Geom &g, const BlockPos &p, const uint8_t *img, int64_t stride, int quality, int16_t zz[64]) {
  long ws[64];
  for (int t = 0; t < 8; ++t) {
    long d[8];
    for (int c = 0; c < 8; ++c) d[c] = block_sample(g, p, img, stride, t, c);
    fdct8(d, true);
    for (int c = 0; c < 8; ++c) ws[t * 8 + c] = d[c];
  }
  for (int c = 0; c < 8; ++c) {
    long d[8];
    for (int r = 0; r < 8; ++r) d[r] = ws[r * 8 + c];
    fdct8(d, false);
    for (int r = 0; r < 8; ++r) {
      const int n = r * 8 + c;
      const int v = quantize(d[r], quant_value(quality, p.comp ? 1 : 0, n));
      zz[zigzag_inv(n)] = (int16_t)((p.dummy && n) ? 0 : v);
    }
  }
}

// T.81 Annex K.3 tables.  tbl: 0 DC luminance, 1 DC chrominance, 2 AC luminance, 3 AC chrominance.
YMI_EHD int huff_nvals(int tbl) { return tbl < 2 ? 12 : 162; }
YMI_EHD int huff_bits(int tbl, int l) {       // number of codes of length l + 1
  const uint8_t b[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                            {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                            {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                            {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
  return b[tbl][l];
}
YMI_EHD int huff_val(int tbl, int j) {        // j-th symbol in code order
  if (tbl < 2) return j;
  const uint8_t v[2][162] = {
      {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
       0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
       0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
       0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
       0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
       0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
       0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
       0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
      {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
       0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
       0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
       0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
       0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
       0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
       0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
       0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
  return v[tbl - 2][j];
}
// j-th symbol of table tbl (code order) -> (symbol, code << 5 | length): the canonical code of T.81 Annex C
YMI_EHD void huff_entry(int tbl, int j, int &symbol, uint32_t &entry) {
  int code = 0, k = 0, l = 1;
  for (; l <= 16; ++l) {
    const int n = huff_bits(tbl, l - 1);
    if (j < k + n) { code += j - k; break; }
    code = (code + n) << 1;
    k += n;
  }
  symbol = huff_val(tbl, j);
  entry = ((uint32_t)code << 5) | (uint32_t)l;
}
// tab [4][256], zero = no code for that symbol
YMI_EHD void huff_fill(uint32_t *tab, int first, int step) {
  for (int i = first; i < 4 * 256; i += step) tab[i] = 0;
}
YMI_EHD void huff_put(uint32_t *tab, int tbl, int j) {
  int s;
  uint32_t e;
  huff_entry(tbl, j, s, e);
  tab[tbl * 256 + s] = e;
}

YMI_EHD int bit_length(unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return 32 - __clz((int)v);
#else
  int n = 0;
  while (v) { ++n; v >>= 1; }
  return n;
#endif
}

// coefficient k (zigzag order) of a block held as 32 packed pairs (little endian)
YMI_EHD int coef_at(const uint32_t pk[32], int k) { return (int)(int16_t)((pk[k >> 1] >> (16 * (k & 1))) & 0xFFFF); }

// jchuff.c encode_one_block.  Sink: put(code, nbits), nbits <= 16.  The bit COUNT and the bits come from this one function.
template <class Sink>
YMI_EHD void encode_block(const uint32_t pk[32], int pred, const uint32_t *dc_tab, const uint32_t *ac_tab, Sink &s) {
  int v = coef_at(pk, 0) - pred;
  int m = v < 0 ? -v : v, lo = v < 0 ? v - 1 : v;
  int nb = bit_length((unsigned)m);
  uint32_t e = dc_tab[nb];
  s.put(e >> 5, (int)(e & 31));
  if (nb) s.put((uint32_t)lo & ((1u << nb) - 1), nb);
  int run = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 1; k < 64; ++k) {
    v = coef_at(pk, k);
    if (v == 0) { ++run; continue; }
    while (run > 15) {
      e = ac_tab[0xF0];
      s.put(e >> 5, (int)(e & 31));
      run -= 16;
    }
    m = v < 0 ? -v : v; lo = v < 0 ? v - 1 : v;
    nb = bit_length((unsigned)m);
    e = ac_tab[((run << 4) | nb) & 255];
    s.put(e >> 5, (int)(e & 31));
    s.put((uint32_t)lo & ((1u << nb) - 1), nb);
    run = 0;
  }
  if (run) {
    e = ac_tab[0];
    s.put(e >> 5, (int)(e & 31));
  }
}

struct CountSink {
  uint32_t n;
  YMI_EHM void put(uint32_t, int nbits) { n += (uint32_t)nbits; }
};

}  // namespace ymi_jpeg_enc
