// Host side shared by the two weight-gradient entries over ymi_conv_wgrad_desc, ymi_conv_wgrad_nhwc_f32 (conv_train.hip) and
// ymi_conv_wgrad_nhwc_h2 (conv_wgrad_h2.hip): what a descriptor must satisfy and how its positions are cut into blocks.  One
// definition, so that the two entries accept and reject the same descriptors with the same codes.
#pragma once
#include "grad_common.h"
#include "../../include/yolact_amd.h"

// the map of g: H x W at stride 1 (the field is 0 or 1), (H + 2 pad - kh) / 2 + 1 at stride 2
static inline int wgrad_out(const ymi_conv_wgrad_desc *d, int size, int k) { return d->stride == 2 ? (size + 2 * d->pad - k) / 2 + 1 : size; }
static inline long wgrad_positions(const ymi_conv_wgrad_desc *d) { return (long)d->B * wgrad_out(d, d->H, d->kh) * wgrad_out(d, d->W, d->kw); }

static inline int validate_wgrad(const ymi_conv_wgrad_desc *d) {
  if (!d) return YMI_ENULL;
  if (d->B < 1 || d->H < 1 || d->W < 1 || d->Cin < 1 || d->Cout < 1) return YMI_EARG;
  if (!((d->kh == 3 && d->kw == 3 && d->pad == 1) || (d->kh == 1 && d->kw == 1 && d->pad == 0))) return YMI_EARG;
  if (d->stride < 0 || d->stride > 2) return YMI_EARG;
  if (d->Cin % 32 != 0 || d->ldg < d->Cout) return YMI_ESHAPE;
  const long P = (long)d->B * d->H * d->W;
  if (P * d->Cin >= (1L << 29) || wgrad_positions(d) * d->ldg >= (1L << 29) || (long)d->kh * d->kw * d->Cin * d->Cout >= (1L << 31)) return YMI_ESHAPE;
  return YMI_OK;
}

struct WgPlan { int nt, gx, gz, nchunks; long per; };

// the decomposition for a validated shape: about 1024 blocks, the (tap, 32 input channels) blocks counted even for a bias alone
static inline WgPlan wgrad_plan(const ymi_conv_wgrad_desc *d) {
  const ymi_wgrad_tiles t = ymi_wgrad_nt(d->Cout);
  const int gx = d->kh * d->kw * (d->Cin / 32);
  const ymi_chunks c = ymi_chunk_plan(wgrad_positions(d), 1024, (long)gx * t.gz);
  return {t.nt, gx, t.gz, c.nchunks, c.per};
}
