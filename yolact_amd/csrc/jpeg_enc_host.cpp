// Host half of the JPEG encoder (eval.py evalimage / evalimages / evalvideo: cv2.imwrite(save_path, img_numpy)): the file header
// SOI .. SOS exactly as libjpeg writes it after jpeg_set_defaults + jpeg_set_quality(q, TRUE) for a 3-component 8-bit image, the
// quantisation tables, and the workspace layout of the device half (jpeg_enc.hip).  Tables come from jpeg_enc_math.h, the same
// functions the kernels call, so header and scan cannot disagree.  No device code in this file; no allocation.
#include "../../include/yolact_amd.h"
#include "jpeg_enc_math.h"
#include <string.h>

using namespace ymi_jpeg_enc;

namespace {

bool valid(int h, int w, int quality, int sub) {
  return h >= 1 && h <= 65535 && w >= 1 && w <= 65535 && quality >= 1 && quality <= 100 && (sub == SUB_420 || sub == SUB_444);
}

int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

}  // namespace

extern "C" {

// Workspace of ymi_jpeg_encode_bgr_u8 (YMI_WS_JPEG_ENC), every part 256-byte aligned:
//   off[0] coefficients int16 [nblk][64]            off[1] bit offset of a block inside its group of 256, uint32 [nblk]
//   off[2] bits per group uint32 [ngrp]             off[3] bit offset of a group uint64 [ngrp]
//   off[4] totals uint64 [2] (scan bits, 0xFF count)
//   off[5] unstuffed scan, raw_bytes = 208 * nblk rounded up to whole 4096-byte chunks
//   off[6] 0xFF bytes per chunk uint32 [nchunk]     off[7] stuffing offset of a chunk uint64 [nchunk]
// Returns the total, or a negative YMI_E* code.  out_bound: scan + stuffing + EOI.
int64_t ymi_jpeg_enc_layout(int h, int w, int sub, int64_t off[8], int64_t *out_bound) {
  if (!valid(h, w, 50, sub)) return -1;
  const Geom g = make_geom(h, w, sub);
  const int64_t ngrp = (g.nblk + 255) / 256;
  const int64_t raw = (g.nblk * MAX_BLOCK_BYTES + 4095) / 4096 * 4096;
  const int64_t nchunk = raw / 4096;
  int64_t o = 0;
  off[0] = o; o = align256(o + g.nblk * 128);
  off[1] = o; o = align256(o + g.nblk * 4);
  off[2] = o; o = align256(o + ngrp * 4);
  off[3] = o; o = align256(o + ngrp * 8);
  off[4] = o; o = align256(o + 16);
  off[5] = o; o = align256(o + raw);
  off[6] = o; o = align256(o + nchunk * 4);
  off[7] = o; o = align256(o + nchunk * 8);
  // every coded block is at most 1660 bits (jpeg_enc_math.h MAX_BLOCK_BYTES), byte stuffing at most doubles a byte, EOI is two
  if (out_bound) *out_bound = 2 * g.nblk * MAX_BLOCK_BYTES + 2;
  return o;
}

int ymi_jpeg_enc_qtables(int quality, uint16_t *qt) {
  if (!qt) return -3;
  if (quality < 1 || quality > 100) return -1;
  for (int t = 0; t < 2; ++t)
    for (int n = 0; n < 64; ++n) qt[t * 64 + n] = (uint16_t)quant_value(quality, t, n);
  return 0;
}

int ymi_jpeg_write_header(int h, int w, int quality, int subsampling, uint8_t *out, size_t cap, size_t *n) {
  if (!out || !n) return -3;
  if (!valid(h, w, quality, subsampling)) return -1;
  uint8_t b[YMI_JPEG_HEADER_BYTES];
  size_t p = 0;
  auto put = [&](int v) { b[p++] = (uint8_t)v; };
  auto put16 = [&](int v) { put(v >> 8); put(v & 255); };
  put16(0xFFD8);
  put16(0xFFE0); put16(16);
  for (const char *s = "JFIF"; *s; ++s) put(*s);
  put(0); put(1); put(1); put(0); put16(1); put16(1); put(0); put(0);
  for (int t = 0; t < 2; ++t) {
    put16(0xFFDB); put16(67); put(t);
    for (int k = 0; k < 64; ++k) put(quant_value(quality, t, zigzag(k)));
  }
  put16(0xFFC0); put16(17); put(8); put16(h); put16(w); put(3);
  put(1); put(subsampling == SUB_420 ? 0x22 : 0x11); put(0);
  put(2); put(0x11); put(1);
  put(3); put(0x11); put(1);
  const int order[4] = {0, 2, 1, 3}, id[4] = {0x00, 0x01, 0x10, 0x11};      // DC lum, AC lum, DC chroma, AC chroma
  for (int i = 0; i < 4; ++i) {
    const int t = order[i], nv = huff_nvals(t);
    put16(0xFFC4); put16(19 + nv); put(id[t]);
    for (int l = 0; l < 16; ++l) put(huff_bits(t, l));
    for (int j = 0; j < nv; ++j) put(huff_val(t, j));
  }
  put16(0xFFDA); put16(12); put(3);
  put(1); put(0x00); put(2); put(0x11); put(3); put(0x11);
  put(0); put(63); put(0);
  if (p != YMI_JPEG_HEADER_BYTES) return -1;
  if (cap < p) return -1;
  memcpy(out, b, p);
  *n = p;
  return 0;
}

}
