// Host emulation of ymi_jpeg_encode_bgr_u8 for the CPU tests (tests/test_jpeg_encode.py builds it with g++): loops over the
// blocks of the scan calling the SAME inline arithmetic and code tables the GPU kernels call (yolact_amd/csrc/jpeg_enc_math.h),
// then packs the bits serially.  Test infrastructure — never part of the product.
#include "../yolact_amd/csrc/jpeg_enc_math.h"
#include <string.h>
#include <vector>

using namespace ymi_jpeg_enc;

namespace {

struct ByteSink {
  uint8_t *out;
  int64_t cap, n = 0;
  uint64_t acc = 0;
  int cnt = 0;
  bool overflow = false;
  void byte(int b) {
    if (n < cap) out[n] = (uint8_t)b; else overflow = true;
    ++n;
  }
  void put(uint32_t code, int nbits) {
    acc = (acc << nbits) | code;
    cnt += nbits;
    while (cnt >= 8) {
      const int b = (int)((acc >> (cnt - 8)) & 0xFF);
      byte(b);
      if (b == 0xFF) byte(0);
      cnt -= 8;
    }
    acc &= (1ull << cnt) - 1;
  }
};

}  // namespace

// Writes the stuffed scan + EOI into out [cap]; returns its length (-1: cap too small).  coefs (may be null): [nblk][64] int16,
// scan order, zigzag order inside a block — what the device keeps in its workspace.
extern "C" int64_t emul_jpeg_encode_bgr_u8(const uint8_t *img, int h, int w, int64_t stride, int quality, int sub, uint8_t *out,
                                           int64_t cap, int16_t *coefs) {
  const Geom g = make_geom(h, w, sub);
  std::vector<int16_t> zz((size_t)g.nblk * 64);
  for (int64_t sb = 0; sb < g.nblk; ++sb) fdct_quant_block(g, block_of(g, sb), img, stride, quality, &zz[(size_t)sb * 64]);
  if (coefs) memcpy(coefs, zz.data(), zz.size() * sizeof(int16_t));
  uint32_t tab[4 * 256];
  huff_fill(tab, 0, 1);
  for (int t = 0; t < 4; ++t)
    for (int j = 0; j < huff_nvals(t); ++j) huff_put(tab, t, j);
  ByteSink s{out, cap};
  for (int64_t sb = 0; sb < g.nblk; ++sb) {
    const BlockPos p = block_of(g, sb);
    uint32_t pk[32];
    memcpy(pk, &zz[(size_t)sb * 64], 128);
    const int pred = p.prev >= 0 ? zz[(size_t)p.prev * 64] : 0;
    CountSink c{0};
    encode_block(pk, pred, tab + (p.comp ? 256 : 0), tab + (p.comp ? 768 : 512), c);
    if (c.n > (uint32_t)MAX_BLOCK_BYTES * 8) return -2;      // the bound YMI_WS_JPEG_ENC_OUT rests on
    encode_block(pk, pred, tab + (p.comp ? 256 : 0), tab + (p.comp ? 768 : 512), s);
  }
  if (s.cnt) s.put((1u << (8 - s.cnt)) - 1, 8 - s.cnt);
  s.byte(0xFF); s.byte(0xD9);
  return s.overflow ? -1 : s.n;
}
