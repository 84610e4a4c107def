// Version / error strings of the C ABI (no device code here).
#include "../../include/yolact_amd.h"
#include <hip/hip_runtime_api.h>

extern "C" {

int64_t ymi_detect_greedy_layout(const ymi_detect_desc *d, int64_t off[4]);   // csrc/detect_greedy.hip
int64_t ymi_jpeg_enc_layout(int h, int w, int sub, int64_t off[8], int64_t *out_bound);   // csrc/jpeg_enc_host.cpp
int64_t ymi_mask_loss_ws_bytes(const ymi_mask_loss_desc *d);                  // csrc/mask_loss.hip
int64_t ymi_match_ws_bytes(const ymi_match_desc *d);                          // csrc/match.hip
int64_t ymi_box_loss_ws_bytes(const ymi_match_desc *d);                       // csrc/match.hip
int64_t ymi_class_loss_ws_bytes(const ymi_class_loss_desc *d);                // csrc/class_loss.hip
int64_t ymi_segm_loss_ws_bytes(const ymi_segm_loss_desc *d);                  // csrc/segm_loss.hip
int64_t ymi_maskiou_input_ws_bytes(const ymi_maskiou_input_desc *d);          // csrc/maskiou_loss.hip
int64_t ymi_conv_bwd_ws_bytes(const ymi_conv_bwd_desc *d);                    // csrc/maskiou_loss.hip
int64_t ymi_maskiou_head_ws_bytes(const ymi_maskiou_head_desc *d);            // csrc/maskiou_loss.hip
int64_t ymi_conv_wgrad_ws_bytes(const ymi_conv_wgrad_desc *d);                // csrc/conv_train.hip
int64_t ymi_bn_ws_bytes(const ymi_bn_desc *d);                                // csrc/bn_train.hip
int64_t ymi_stem_wgrad_ws_bytes(const ymi_stem_wgrad_desc *d);                // csrc/stem_train.hip
int64_t ymi_augment_ws_bytes(const ymi_augment_desc *d);                      // csrc/augment.hip
int64_t ymi_preconv_wgrad_ws_bytes(const ymi_preconv_wgrad_desc *d);          // csrc/darknet_train.hip
int64_t ymi_conv_wgrad_h2_ws_bytes(const ymi_conv_wgrad_desc *d);             // csrc/conv_wgrad_h2.hip
int64_t ymi_coco_mask_ws_bytes(const ymi_coco_mask_desc *d);                  // csrc/coco_mask.hip

int ymi_abi_version(void) { return YMI_ABI_VERSION; }

const char *ymi_strerror(int code) {
  switch (code) {
    case 0: return "ok";
    case -1: return "bad argument / unsupported configuration";
    case -2: return "shape or alignment constraint violated";
    case -3: return "null pointer";
    case YMI_EFORMAT: return "corrupt or truncated input stream";
    case YMI_EUNSUPPORTED: return "valid input outside the supported subset";
  }
  if (code > 0) return hipGetErrorString((hipError_t)code);
  return "unknown error";
}

// Workspace sizes in bytes: the one place the formulas of the header comments are written down as code, so that a host other than
// the Python shim does not re-derive them (SURVEY 8(b) "ownership": the caller allocates, the library never does).
int64_t ymi_workspace_bytes(int what, const void *desc) {
  auto cdiv = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
  if (what == YMI_WS_AMAX_SLOT) return (int64_t)YMI_AMAX_SUB * YMI_AMAX_STRIDE * 4;
  if (!desc) return -3;
  switch (what) {
    case YMI_WS_WINO_V:
    case YMI_WS_WINO_M: {
      const ymi_wino_desc *d = (const ymi_wino_desc *)desc;
      const int m = d->m == 4 ? 4 : 2;
      int64_t G = (int64_t)(m + 2) * (m + 2), T = 0;
      if (d->nlev != 0) {          // level table: the tiles of every level, one after the other
        if (d->nlev < 2 || d->nlev > 5 || d->m != 4 || d->B < 1 || d->C < 1 || d->Cout < 1) return -1;
        for (int l = 0; l < d->nlev; ++l) {
          if (d->lev[l].H < 1 || d->lev[l].W < 1) return -1;
          T += (int64_t)d->B * cdiv(d->lev[l].H, 4) * cdiv(d->lev[l].W, 4);
        }
        return 4 * G * T * (what == YMI_WS_WINO_V ? (int64_t)d->C : cdiv(d->Cout, 4) * 4);
      }
      if ((d->m != 0 && d->m != 2 && d->m != 4) || d->B < 1 || d->H < 1 || d->W < 1 || d->C < 1 || d->Cout < 1) return -1;
      T = (int64_t)d->B * cdiv(d->H, m) * cdiv(d->W, m);
      return 4 * G * T * (what == YMI_WS_WINO_V ? (int64_t)d->C : cdiv(d->Cout, 4) * 4);
    }
    case YMI_WS_SPLITK: {
      const ymi_conv_desc *d = (const ymi_conv_desc *)desc;
      if (d->B < 1 || d->Ho < 1 || d->Wo < 1 || d->Cout < 1 || d->split_k < 0) return -1;
      return d->split_k > 1 ? 4 * (int64_t)d->split_k * d->B * d->Ho * d->Wo * d->Cout : 0;
    }
    case YMI_WS_MASK_IOU: {
      const ymi_mask_iou_shape *d = (const ymi_mask_iou_shape *)desc;
      if (d->A < 0 || d->B < 0) return -1;
      return 4 * ((int64_t)d->A * d->B + d->A + d->B);
    }
    case YMI_WS_JPEG_COEFS: return 2 * ((const ymi_jpeg_info *)desc)->coef_count;
    case YMI_WS_JPEG_PLANES: return ((const ymi_jpeg_info *)desc)->plane_bytes;
    case YMI_WS_DETECT_SCORES_T:
    case YMI_WS_DETECT_PER_PRIOR:
    case YMI_WS_DETECT_CAND:
    case YMI_WS_DETECT_REC: {
      const ymi_detect_desc *d = (const ymi_detect_desc *)desc;
      if (d->B < 1 || d->P < 1 || d->C < 2 || d->D < 0 || d->top_k < 1 || d->max_det < 1) return -1;
      if (what == YMI_WS_DETECT_SCORES_T) return 4 * (int64_t)d->B * (d->C - 1) * d->P;
      if (what == YMI_WS_DETECT_PER_PRIOR) return 4 * (int64_t)d->B * d->P;
      if (what == YMI_WS_DETECT_CAND) return 4 * (int64_t)d->B * (d->C - 1) * d->top_k;
      const int64_t cap = d->cross_class ? d->top_k : d->max_det;
      return 4 * (int64_t)d->B * (1 + cap * (6 + d->D));
    }
    case YMI_WS_DETECT_GREEDY: {
      const ymi_detect_desc *d = (const ymi_detect_desc *)desc;
      if (d->B < 1 || d->P < 1 || d->C < 2 || d->max_det < 1) return -1;
      int64_t off[4];
      return ymi_detect_greedy_layout(d, off);
    }
    case YMI_WS_JPEG_ENC:
    case YMI_WS_JPEG_ENC_OUT: {
      const ymi_jpeg_enc_desc *d = (const ymi_jpeg_enc_desc *)desc;
      int64_t off[8], bound = 0;
      const int64_t total = ymi_jpeg_enc_layout(d->h, d->w, d->subsampling, off, &bound);
      return total < 0 ? total : (what == YMI_WS_JPEG_ENC ? total : bound);
    }
    case YMI_WS_MASK_LOSS: return ymi_mask_loss_ws_bytes((const ymi_mask_loss_desc *)desc);
    case YMI_WS_MATCH: return ymi_match_ws_bytes((const ymi_match_desc *)desc);
    case YMI_WS_BOX_LOSS: return ymi_box_loss_ws_bytes((const ymi_match_desc *)desc);
    case YMI_WS_CLASS_LOSS: return ymi_class_loss_ws_bytes((const ymi_class_loss_desc *)desc);
    case YMI_WS_SEGM_LOSS: return ymi_segm_loss_ws_bytes((const ymi_segm_loss_desc *)desc);
    case YMI_WS_MASKIOU_INPUT: return ymi_maskiou_input_ws_bytes((const ymi_maskiou_input_desc *)desc);
    case YMI_WS_CONV_BWD: return ymi_conv_bwd_ws_bytes((const ymi_conv_bwd_desc *)desc);
    case YMI_WS_MASKIOU_HEAD: return ymi_maskiou_head_ws_bytes((const ymi_maskiou_head_desc *)desc);
    case YMI_WS_CONV_WGRAD: return ymi_conv_wgrad_ws_bytes((const ymi_conv_wgrad_desc *)desc);
    case YMI_WS_BN: return ymi_bn_ws_bytes((const ymi_bn_desc *)desc);
    case YMI_WS_STEM_WGRAD: return ymi_stem_wgrad_ws_bytes((const ymi_stem_wgrad_desc *)desc);
    case YMI_WS_AUGMENT: return ymi_augment_ws_bytes((const ymi_augment_desc *)desc);
    case YMI_WS_PRECONV_WGRAD: return ymi_preconv_wgrad_ws_bytes((const ymi_preconv_wgrad_desc *)desc);
    case YMI_WS_CONV_WGRAD_H2: return ymi_conv_wgrad_h2_ws_bytes((const ymi_conv_wgrad_desc *)desc);
    case YMI_WS_COCO_MASK: return ymi_coco_mask_ws_bytes((const ymi_coco_mask_desc *)desc);
    case YMI_WS_RLE_COUNTS: {
      const ymi_rle_shape *d = (const ymi_rle_shape *)desc;
      if (d->N < 0 || d->h < 1 || d->w < 1) return -1;
      const int64_t cap = d->cap > 0 ? d->cap : (int64_t)d->h * d->w + 1;
      return 4 * (int64_t)d->N * cap;
    }
  }
  return -1;
}

}
