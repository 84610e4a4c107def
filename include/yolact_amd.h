/* yolact_amd.h — C ABI of libyolact_amd.so, the MI355X (gfx950) YOLACT inference hot path.
 *
 * Every entry point: plain pointers + sizes, an explicit hipStream_t (passed as void*), returns
 *   0 = ok, negative = argument/shape error (YMI_E*), positive = hipError_t of the launch.
 * The library never allocates or frees device memory: the caller owns every input, output and
 * workspace buffer (SURVEY §8(b) "ownership").  All tensors are float32 unless stated, device
 * pointers, densely packed in the layout named in the comment.  Activations are NHWC.
 *
 * Each function cites the reference interface (file:line under dbolya/yolact) it replaces.
 */
#ifndef YOLACT_AMD_H
#define YOLACT_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YMI_ABI_VERSION 9

/* negative return codes (ymi_strerror) */
#define YMI_EFORMAT (-4)       /* corrupt or truncated input stream (ymi_jpeg_*) */
#define YMI_EUNSUPPORTED (-5)  /* valid input outside the supported subset (ymi_jpeg_*) */

/* activation codes (epilogue) */
enum { YMI_ACT_NONE = 0, YMI_ACT_RELU = 1, YMI_ACT_LEAKY01 = 2, YMI_ACT_TANH = 3, YMI_ACT_SIGMOID = 4 };
/* residual modes */
enum { YMI_RES_NONE = 0, YMI_RES_ADD = 1, YMI_RES_BILINEAR = 2 };

/* One output segment of a convolution: output channels [n0,n1) of pixel (b,pix) go to
 *   ptr + b*batch_stride + pix*row_stride + (n - n0)      (element units)
 * so a single GEMM can scatter to several tensors (the three shared prediction-head convs,
 * yolact.py:169-173, become one GEMM with Cout = A*4 + A*81 + A*32) and can write straight
 * into the level-concatenated [B, P, k] tensors (yolact.py:633-634) without a torch.cat. */
typedef struct {
  int32_t n0, n1;
  int32_t act;          /* YMI_ACT_* applied to this segment */
  int32_t row_stride;   /* elements between consecutive output pixels */
  int64_t batch_stride; /* elements between consecutive images */
  float *ptr;
} ymi_conv_seg;

/* Fused convolution descriptor.
 * Replaces nn.Conv2d [+ BatchNorm2d (eval)] [+ residual add | FPN top-down bilinear add] [+ activation]:
 *   backbone.py:37-57 (Bottleneck), :126-139 (stem), :222-236 (darknet unit), yolact.py:319-361 (FPN),
 *   utils/functions.py:163-213 (make_net convs), yolact.py:146-193 (prediction heads).
 * y[b,oy,ox,n] = act( scale[n] * sum_{ky,kx,c} x[b, oy*s-p+ky, ox*s-p+kx, c] * w[n,ky,kx,c] + bias[n]  (+ res) )
 * fp32 in, fp32 accumulate, fp32 out.  The products are formed by the tile `tile` selects: plain ids = v_mfma_f32_32x32x2_f32
 * (exact fp32 products); `| YMI_TILE_X3` = three-piece bf16 split; `| YMI_TILE_H2` = two-piece fp16 split (see the enum). */
typedef struct {
  const float *x;       /* [B,H,W,ldx] NHWC; channels [0,Cin) of each pixel are used; 16-byte aligned, < 2 GiB */
  const float *w;       /* packed [CoutPad][Kpad], k = (ky*kw+kx)*Cin + c; CoutPad % 128 == 0, Kpad % 32 == 0, zero padded */
  const float *scale;   /* [Cout] or NULL (=1)  — folded BatchNorm gamma/sqrt(var+eps) */
  const float *bias;    /* [Cout] or NULL (=0)  — conv bias or folded BatchNorm shift */
  const float *res;     /* residual source or NULL */
  int32_t B, H, W, Cin, ldx;
  int32_t Ho, Wo, Cout;
  int32_t kh, kw, stride, pad;
  int32_t Kpad;
  int32_t res_mode;     /* YMI_RES_* */
  int32_t res_ld;       /* channel stride of res pixels */
  int32_t res_H, res_W; /* source size for YMI_RES_BILINEAR (res is [B,res_H,res_W,res_ld]) */
  int32_t res_after_act;/* 1: y = act(conv) + res (darknet block, backbone.py:214-215); 0: y = act(conv + res) */
  int32_t nseg;         /* 1..3 */
  int32_t tile;         /* 0 = auto; else YMI_TILE_* override (tests / tuning) */
  int32_t cin_alg;      /* real (un-padded) input channels for FLOP accounting; 0 = Cin */
  int32_t split_k;      /* 0 / 1: off.  S > 1: 1x1 convolutions (and the pipelined DCN tiles, YMI_TILE_DCNP) only — the K = Cin reduction is cut into S ranges computed by S
                         * times as many blocks (small maps, long K: too few output tiles to fill 256 CUs otherwise); the
                         * partial sums go through `split_ws` and are added in a fixed order (deterministic) by a second
                         * launch that applies scale / bias / residual / activation.  Needs (Kpad / 32) % S == 0, one dense
                         * output segment, activation none / ReLU / LeakyReLU, residual none / add. */
  ymi_conv_seg seg[3];
  const void *w_x3;     /* optional, for tile | YMI_TILE_X3: the SAME filters pre-split into three bf16 planes
                         * [3][CoutPad][Kpad] (uint16 bit patterns; plane 0 = top 8 significant bits by truncation, 1 = next 8,
                         * 2 = last 8; plane0 + plane1 + plane2 == w exactly).  With it the kernel splits only the activations
                         * on the fly (a third of the VALU work); NULL: both operands are split on the fly. */
  float *split_ws;      /* split_k > 1: workspace of split_k * B*Ho*Wo * Cout floats, 16-byte aligned */
  int32_t cout_alg;     /* real output channels for FLOP accounting when Cout carries zero-filter padding columns; 0 = Cout */
  int32_t _pad2;
  /* -- fp16x2 tiles (tile | YMI_TILE_H2) ------------------------------------------------------------------------------
   * w_h2: the SAME filters as two fp16 planes [2][CoutPad][Kpad] (uint16 bit patterns): row n is scaled by the power of two
   * sW[n] that maps max|w[n,:]| into [2^13, 2^14); plane 0 = fp16(w * sW) (round to nearest), plane 1 = fp16(w * sW - plane 0).
   * scale_h2[n] = scale[n] / sW[n]  (or 1 / sW[n] without a scale): the epilogue's per-channel factor with the filter scale
   * folded in (exact: a power of two).  winv_h2[n] = 1 / sW[n] alone (partial sums of split-K launches).
   * x_amax: DEVICE magnitude-bound slot of the input tensor: YMI_AMAX_SUB (16) floats, YMI_AMAX_STRIDE (64) floats apart
   * (4 KB per slot), whose MAXIMUM is an upper bound on |x| — raised by the launch that produced x (its y_amax) or by
   * ymi_amax_f32, zeroed by the caller before that launch; the kernel scales x by the power of two sA that maps
   * bound * x_amax_mul into [2^13, 2^14) before the fp16 split and divides the accumulators by sA.  A bound that is too small
   * can overflow fp16.  (Sub-slots: thousands of waves commit to one tensor's bound; spread over 16 cache lines the atomics
   * of a launch's first residency round cost ~1 us instead of ~50.) */
  const void *w_h2;
  const float *scale_h2;
  const float *winv_h2;
  const float *x_amax;
  float *y_amax;        /* any tile: DEVICE slot (same layout as x_amax) or NULL: raised atomically so that its maximum becomes
                         * max|y| over everything this launch writes.  nseg > 1 (ABI 5): nseg CONSECUTIVE slots (YMI_AMAX_SUB *
                         * YMI_AMAX_STRIDE floats apart), segment k raises slot k — the segments of one launch may be different
                         * tensors with different consumers (the merged head0.upfeature + proto_net[0] launch) */
  float x_amax_mul;     /* static factor on *x_amax; 0 = 1 */
  int32_t _pad3;
} ymi_conv_desc;

/* block tile BMxBN; _Kn = the block's 4 waves also split K n ways (partial sums reduced in LDS in a fixed order:
 * deterministic, but a different fp32 summation order than the unsplit tiles) */
enum { YMI_TILE_AUTO = 0, YMI_TILE_128x128 = 1, YMI_TILE_128x64 = 2, YMI_TILE_64x64 = 3, YMI_TILE_128x32 = 4,
       YMI_TILE_64x128 = 5, YMI_TILE_32x32_K4 = 6, YMI_TILE_64x32_K2 = 7, YMI_TILE_32x64_K2 = 8,
       /* _Sn = n-stage LDS pipeline (n-1 K steps of LDS-DMA in flight); Cin % 32 == 0 layers only */
       YMI_TILE_64x64_S3 = 9, YMI_TILE_64x64_S4 = 10, YMI_TILE_64x128_S3 = 11, YMI_TILE_128x64_S3 = 12,
       YMI_TILE_32x32_K4_S4 = 13, YMI_TILE_64x32_K2_S3 = 14, YMI_TILE_32x64_K2_S3 = 15,
       /* _W8 = 512-thread blocks (8 waves): half the global->LDS traffic per FLOP of the 4-wave tile of equal wave tile */
       YMI_TILE_128x128_W8 = 16, YMI_TILE_256x128_W8 = 17, YMI_TILE_128x256_W8 = 18,
       /* one block per CU, deep LDS-DMA pipeline (96 - 144 KB of stages): the regime the bf16x3 variants need, whose K
        * step is too short to hide a DMA round trip behind one or two co-resident blocks */
       YMI_TILE_128x128_S3 = 19, YMI_TILE_128x128_W8_S3 = 20, YMI_TILE_256x128_W8_S3 = 21, YMI_TILE_128x128_W8_S4 = 22,
       /* round 6, ymi_conv3x3_winograd_f32 only (`| YMI_TILE_H2`, v_planes = 1): the grouped GEMM of the Winograd path as ONE persistent
        * producer / consumer launch over (component, 128-row tile, 256-column block) work items whose chunk stream does not stop at item
        * boundaries (csrc/wgemm.hip); M is bit-identical to the 128 x 128 tile's */
       YMI_TILE_WG_128x256 = 23,
       /* tile | YMI_TILE_X3: the same block tile computed as "bf16x3" — every fp32 operand split exactly into three bf16
        * pieces BY TRUNCATION (24 mantissa bits), 6 of the 9 piece products on v_mfma_f32_32x32x16_bf16 with fp32
        * accumulation; the dropped terms (m*l, l*m, l*l) are < 2^-21 |a b| in the worst case (|m| < 2^-7 |a|, |l| < 2^-15 |a|;
        * simulated maximum 6.4 * 2^-24) and, because truncated pieces carry the sign of their operand, always of the sign of
        * a*b: a one-sided error of +0.63 * 2^-24 |a b| on average.  Cin % 32 == 0
        * layers; available for tiles 1, 2, 3, 5, 6, 7, 8, 9, 11, 12, 16, 17, 19 - 22. */
       YMI_TILE_X3 = 32,
       /* tile | YMI_TILE_H2: the same block tile computed as "fp16x2" — x * s = h + l with two fp16 pieces taken by ROUND TO
        * NEAREST (11 + 11 significant bits + two signs: about two thirds of all fp32 values are represented exactly, the rest
        * with an error of one fp32 ulp; unbiased), s a power of two per tensor (activations, from x_amax) or per filter row;
        * 3 of the 4 piece products (h*l, l*h, h*h) on v_mfma_f32_32x32x16_f16 with fp32 accumulation; the dropped l*l term is
        * <= 2^-22 |a b|, unbiased.  Half the matrix-pipe work of X3 and no byte permutes in the split.  Needs w_h2, scale_h2,
        * x_amax.  Same base tiles as X3. */
       YMI_TILE_H2 = 64,
       /* YMI_TILE_H2 | YMI_TILE_DCNP | YMI_DCNP_* (ymi_dcn_v2_forward_f32 only): the software-pipelined gather-GEMM of
        * csrc/dcn.hip — corner loads three K chunks ahead in a register ring, every sample formed once per row block and stored
        * to LDS as the two fp16 planes, no operand split in the MFMA loop.  The low five bits select ITS block tile (enum
        * below), not a YMI_TILE_* of the conv engine.  One dense output, activation none / ReLU / LeakyReLU, no residual. */
       YMI_TILE_DCNP = 128 };
/* block tiles of the pipelined DCN kernel (BM x BN, _W8 = 512-thread blocks) */
enum { YMI_DCNP_64x128 = 1, YMI_DCNP_64x128_W8 = 2, YMI_DCNP_64x64 = 3, YMI_DCNP_128x128_W8 = 4, YMI_DCNP_128x64_W8 = 5,
       YMI_DCNP_32x128 = 6,
       /* 6 / 8 / 10 / 12 waves of 32 x 64, corner loads two chunks ahead (one register slot): one block per CU, rows sized to M / 256 */
       YMI_DCNP_96x128_W6 = 7, YMI_DCNP_128x128_W8_R1 = 8, YMI_DCNP_160x128_W10 = 9, YMI_DCNP_192x128_W12 = 10,
       /* 256 output channels per block (every sample gathered once for all of them): the Cout >= 256 layers, normally with
        * ymi_conv_desc.split_k = S (chunk-aligned K ranges, partial sums through split_ws, deterministic second pass) because their
        * maps are small */
       YMI_DCNP_64x256_W8 = 11, YMI_DCNP_96x256_W12 = 12, YMI_DCNP_128x256_W16 = 13,
       /* 64 x 64 wave tiles (ordinary convolutions only: ymi_conv2d_nhwc_f32) */
       YMI_DCNP_128x256_W8T = 14, YMI_DCNP_128x128_W4T = 15, YMI_DCNP_256x128_W8T = 16,
       /* 32 output channels per block (ordinary convolutions only): the 27-channel conv_offset_mask of a DCN layer
        * (dcn_v2.py:107-112) with its filters zero-padded to 32 — the cost of such a layer is staging its input, so a block
        * spends its waves on rows, not on columns nobody needs */
       YMI_DCNP_128x32_W4 = 17, YMI_DCNP_256x32_W8 = 18, YMI_DCNP_64x32_W2 = 19,
       /* the weight-stationary streaming kernel of csrc/wstat.hip (ordinary convolutions with Cout <= 32 / <= 64, no residual):
        * the filters of the block's K range stay in LDS, every wave streams its own rows from global memory straight into MFMA
        * operand registers, no barrier in the loop.  BM x BN, _W4 / _W8 = waves per block (32 or 64 rows per wave).  The K range
        * of a block must fit 64 KB of LDS: ymi_conv_desc.split_k >= Kpad * BN / 16384 (YMI_EARG otherwise) */
       YMI_DCNP_WS_128x32_W4 = 20, YMI_DCNP_WS_256x32_W8 = 21, YMI_DCNP_WS_256x32_W4 = 22, YMI_DCNP_WS_512x32_W8 = 23,
       YMI_DCNP_WS_128x64_W4 = 24, YMI_DCNP_WS_256x64_W8 = 25, YMI_DCNP_WS_256x64_W4 = 26, YMI_DCNP_WS_512x64_W8 = 27,
       /* round 5, csrc/patch.hip: 3x3 / stride 1 / pad 1, 64 -> 64 channels (conv2 of the first ResNet stage, backbone.py:44-46), one
        * dense output, no residual: a persistent block per CU owns 8 x 16 pixel output tiles, the 10 x 18 x 64 input patch lives in
        * LDS as fp16 planes (loaded ONCE instead of once per filter tap) and the filters live in registers */
       YMI_DCNP_PATCH_C64 = 28,
       /* round 6, csrc/pcconv.hip: the same convolutions as the pipelined tiles (3x3 / pad 1 or 1x1 / pad 0, Cin % 32 == 0, one dense
        * output, optional residual, optional split_k) as a PRODUCER / CONSUMER block: four consumer waves (one per SIMD: fragment
        * reads + MFMAs only) and four producer waves (row requests, the fp32 -> fp16-plane split, the filter LDS-DMAs), so that a
        * request stalled on the vector-memory pipe no longer holds MFMAs back.  BM x BN = the block tile; results are bit-identical
        * to the pipelined tiles' (same products, same order per accumulator) */
       YMI_DCNP_PC_128x128 = 29,
       /* round 6, csrc/patch2.hip: 3x3 / stride 1 / pad 1, Cin % 32 == 0, Cout >= 64, no residual, up to three dense output segments
        * with boundaries at multiples of 128 channels: the input patch of a TH x TW pixel tile (256 / 192 pixels; the shape is picked
        * per map size) lives in LDS one 32-channel chunk at a time, only the filters stream per (chunk, tap) step — the nine taps of a
        * 3x3 convolution read the same pixels, so the A operand crosses the global -> LDS path once instead of nine times */
       YMI_DCNP_PATCH2_256 = 30, YMI_DCNP_PATCH2_192 = 31 };

int ymi_abi_version(void);
const char *ymi_strerror(int code);

/* -- convolution engine ---------------------------------------------------------------- */
int ymi_conv2d_nhwc_f32(const ymi_conv_desc *d, void *stream);
/* algorithmic FLOPs (2*MACs) of a descriptor — used by bench.py's roofline accounting */
double ymi_conv_flops(const ymi_conv_desc *d);
/* which tile the auto heuristic picks (YMI_TILE_*) */
int ymi_conv_pick_tile(const ymi_conv_desc *d);

/* Winograd F(2x2,3x3) variant of ymi_conv2d_nhwc_f32 for kh = kw = 3, stride 1, pad 1, Cin % 32 == 0, Cout % 4 == 0, no
 * residual, one dense output, activation none / ReLU / LeakyReLU (nn.Conv2d 3x3 + BN + ReLU of backbone.py:37-57,
 * yolact.py:319-361, utils/functions.py:163-213).  2.25x fewer multiplications; results differ from the direct kernel by
 * fp32 rounding of the transforms only (<= 2e-6 relative).
 * u: transformed filters [G][CoutPad][C] (U = G g G^T, CoutPad % 128 == 0, zero padded), V / M: caller workspaces of
 * G*T*C and G*T*ceil(Cout/4)*4 floats with T = B*ceil(H/m)*ceil(W/m), G = (m+2)^2 = 16 (m = 2) or 36 (m = 4; 4x fewer
 * multiplications than the direct kernel, fp32 rounding ~4x that of m = 2, still <= 1e-5 relative).  With nseg > 0 the output transform scatters
 * to segments (the shared prediction-head conv, yolact.py:169-193). */
typedef struct {
  const float *x;       /* [B,H,W,C] NHWC */
  const float *u;
  const float *scale;   /* [Cout] or NULL */
  const float *bias;    /* [Cout] or NULL */
  float *y;             /* [B,H,W,Cout] */
  float *V, *M;
  int32_t B, H, W, C, Cout;
  int32_t act;          /* YMI_ACT_NONE / RELU / LEAKY01 */
  int32_t tile;         /* tile of the 16-group GEMM (0 = auto) */
  int32_t nseg;         /* 0: dense y (Cout % 4 == 0, act none/ReLU/LeakyReLU).  1..3: scatter to seg[] like ymi_conv_desc
                         * (any Cout, any YMI_ACT_* per segment; `y` and `act` are ignored) */
  int32_t m;            /* output tile edge: 0 or 2 = F(2x2,3x3) (16 GEMMs), 4 = F(4x4,3x3) (36 GEMMs) */
  int32_t _pad0;
  ymi_conv_seg seg[3];
  const void *u_x3;     /* optional, for tile | YMI_TILE_X3: u pre-split into bf16 planes [G][3][CoutPad][C] (see ymi_conv_desc.w_x3) */
  int32_t cout_alg;     /* real output channels for FLOP accounting (see ymi_conv_desc.cout_alg); 0 = Cout */
  int32_t v_planes;     /* tile | YMI_TILE_H2 only.  1: the input transform writes V directly as two fp16 planes [G][2][T][C]
                         * (scaled by the power of two derived from x_amax * the transform's gain bound; same bytes as fp32 V) and
                         * the grouped GEMM runs with NO operand split in its loop; 0: V stays fp32 and is split on the fly */
  /* tile | YMI_TILE_H2: u as fp16x2 planes [G][2][CoutPad][C] with one scale per (component, filter row);
   * uinv_h2 [G][CoutPad] = 1 / that scale; x_amax / y_amax as in ymi_conv_desc (y_amax may be NULL) */
  const void *u_h2;
  const float *uinv_h2;
  const float *x_amax;
  float *y_amax;
  /* ABI 4, m = 4 only.  x_up != NULL: the layer's input is F.interpolate(x_up, scale_factor 2, bilinear, align_corners False)
   * (+ ReLU if up_relu) of x_up [B,H/2,W/2,C] (H, W even), evaluated INSIDE the input transform with the operation order of
   * ymi_bilinear_nhwc_f32 (bit-identical to materialising it; `x` is ignored).  Saves the write and the read of the upsampled
   * tensor: protonet's interpolate -> conv (utils/functions.py:187-206, yolact.py:588-599).  x_amax = the bound of x_up. */
  const float *x_up;
  int32_t up_relu, _pad4;
  /* ABI 6, m = 4, nseg = 0, Cout = 256 only.  proj_w_h2 != NULL: the layer's output is consumed by ONE 1x1 convolution to
   * proj_cout <= 32 channels (protonet's last layer, utils/functions.py:163-213: conv3x3 + ReLU -> conv1x1) and nothing else; the
   * output transform multiplies every 4x4 tile by those filters while it is in registers / LDS and writes
   * proj_y [B,H,W,proj_ldy] = act2(conv1x1(act(conv3x3(x)))) — `y` is not written (may be NULL), y_amax is not updated.
   * proj_w_h2 / proj_scale_h2: the 1x1's fp16x2 filter planes [2][128][256] and scale_h2 [128] (ymi_conv_desc.w_h2 / scale_h2 of
   * the same layer); the tile is scaled by a power of two derived from its own maximum, so no magnitude bound of y is needed. */
  const void *proj_w_h2;
  const float *proj_scale_h2, *proj_bias;   /* proj_bias may be NULL */
  float *proj_y, *proj_y_amax;              /* proj_y_amax: magnitude-bound slot of proj_y, may be NULL */
  int32_t proj_cout, proj_ldy, proj_act, _pad5;
  /* Level table (trailing fields, ABI number unchanged; all zero = the launch above).  nlev = 2..5: ONE input transform, ONE
   * grouped GEMM and ONE output transform apply the same filters to nlev feature maps of different sizes (the prediction heads of
   * P4..P7 share their weights: yolact.py:133-212, share_prediction_module).  V / M rows are level-major: all tiles of lev[0] in
   * (b, ty, tx) order, then lev[1], ...; T = B * sum_l ceil(H_l / 4) * ceil(W_l / 4) (also what YMI_WS_WINO_V / _M return).
   * x, y, H, W, x_amax above are ignored; B, C, Cout, act, scale, bias, seg[], tile hold for every level.  Accepted only with
   * m = 4, tile | YMI_TILE_H2 (v_planes 1 or 0), no x_up, no proj_*: anything else is YMI_EARG.
   * The merged V has ONE power-of-two scale, derived from the largest of the levels' bounds.  Where the levels name different
   * x_amax slots the input transform writes that maximum to lev_amax (a slot of the caller's, zeroed like every other slot; required
   * then) and the GEMM reads it there; where they all name the same slot the GEMM reads that slot and lev_amax is not touched.
   * nseg = 0: level l writes its dense y and raises its own y_amax (may be NULL; levels may share one slot).
   * nseg = 1..3: level l writes segment k at (char *)seg[k].ptr + seg_off[k]; y_amax above is raised as in the single launch.
   * Profile: the launch is recorded with the algorithmic FLOPs of lev[0]; the nabs <= 8 layers it absorbed follow as records of
   * kind 12 (abs_flops[i], no duration), so that records keep mapping onto the caller's layer list by position. */
  int32_t nlev, nabs;
  struct {
    const float *x;       /* [B,H,W,C] */
    const float *x_amax;
    float *y, *y_amax;    /* nseg = 0 */
    int64_t seg_off[3];   /* nseg > 0: bytes */
    int32_t H, W;
  } lev[5];
  float *lev_amax;
  double abs_flops[8];
} ymi_wino_desc;
int ymi_conv3x3_winograd_f32(const ymi_wino_desc *d, void *stream);

/* Raises the magnitude-bound slot `out` (ymi_conv_desc.x_amax layout: 16 sub-slots 64 floats apart, 961 floats in all) to
 * max_i |x[i]| over n floats (n % 4 == 0, x 16-byte aligned): the bound of a tensor that no ymi_conv launch produced (the
 * network input).  The caller zeroes the slot beforehand. */
#define YMI_AMAX_SUB 16
#define YMI_AMAX_STRIDE 64
int ymi_amax_f32(const float *x, long n, float *out, void *stream);

/* -- layout / pooling / resize ---------------------------------------------------------- */
/* x [B,C,H,W] (C<=4) -> y [B,H,W,4], zero-filled channels C..3.  Entry of Yolact.forward (yolact.py:564). */
int ymi_nchw_to_nhwc4_f32(const float *x, float *y, int B, int C, int H, int W, void *stream);
/* the same, and raises the magnitude-bound slot `amax` (ymi_amax_f32's layout, zeroed by the caller) to max |x|: one launch
 * for the two passes over the network input */
int ymi_nchw_to_nhwc4_amax_f32(const float *x, float *y, int B, int C, int H, int W, float *amax, void *stream);
/* y [B,H,W,C] NHWC -> x [B,C,H,W] (returning NCHW tensors to callers that expect them) */
int ymi_nhwc_to_nchw_f32(const float *x, float *y, int B, int C, int H, int W, void *stream);
/* nn.MaxPool2d(3, stride 2, pad 1) on NHWC, C % 4 == 0 (backbone.py:80,131). */
int ymi_maxpool3x3s2_nhwc_f32(const float *x, float *y, int B, int H, int W, int C, int Ho, int Wo, void *stream);
/* F.interpolate(mode='bilinear', align_corners=False) on NHWC, C % 4 == 0, optional ReLU
 * (layers/interpolate.py:4-17; utils/functions.py:194). scale_h/scale_w: the 1/scale_factor torch would
 * use (pass 0 to derive in/out like the size= form). */
int ymi_bilinear_nhwc_f32(const float *x, float *y, int B, int Hi, int Wi, int C, int Ho, int Wo,
                          float scale_h, float scale_w, int relu, void *stream);

/* The FPN top-down sum as its own in-place pass (ABI 7; yolact.py:332-334: x = F.interpolate(x, size, bilinear) + lat_layer(convout)):
 *   y [B,Ho,Wo,C] += bilinear(x [B,Hi,Wi,C] -> Ho x Wo),  C % 4 == 0, both 16-byte aligned.
 * Same interpolation (fp32 coordinates, same expression) as the YMI_RES_BILINEAR epilogue of ymi_conv2d_nhwc_f32: a lateral
 * convolution without residual followed by this pass equals the fused launch (bit for bit when the same GEMM tile runs).  What it buys: the lateral convolutions
 * of the lower levels depend only on their backbone stage, so the engine launches them early on its side stream, beside the later
 * (under-filled) backbone stages, and only this small pass stays on the critical path.  y_amax: magnitude-bound slot of the SUM
 * (ymi_conv_desc.x_amax layout; zeroed by the caller; may be NULL). */
int ymi_bilinear_add_nhwc_f32(const float *x, float *y, int B, int Hi, int Wi, int C, int Ho, int Wo, float *y_amax, void *stream);

/* Small direct convolution for FastMaskIoUNet (yolact.py:363-375; config maskiou_net, data/config.py:785-791):
 * x [B,H,W,Cin] NHWC, w [kh*kw*Cin][CoutPad4] (k = (ky*kw+kx)*Cin + c, CoutPad4 = ceil(Cout/4)*4, zero padded),
 * y [B,Ho,Wo,Cout]; optional bias and ReLU. */
int ymi_conv2d_direct_nhwc_f32(const float *x, const float *w, const float *bias, float *y, int B, int H, int W,
                               int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int relu,
                               void *stream);
/* y[b,c] = max_p x[b,p,c]  (F.max_pool2d over the whole map, yolact.py:372) */
int ymi_global_maxpool_nhwc_f32(const float *x, float *y, int B, int HW, int C, void *stream);

/* -- Detect: softmax + decode + Fast NMS (layers/functions/detection.py:32-180) ---------- */
typedef struct {
  const float *conf;    /* [B,P,C] raw class logits if conf_is_logits else post-softmax scores */
  const float *loc;     /* [B,P,4] */
  const float *coef;    /* [B,P,D] mask coefficients (post-tanh) */
  const float *priors;  /* [P,4] cx,cy,w,h */
  int32_t B, P, C, D;   /* C includes background class 0; D = mask_dim */
  int32_t conf_is_logits;
  int32_t top_k;        /* cfg.nms_top_k (200), <= 256 */
  int32_t max_det;      /* cfg.max_num_detections (100), <= 256 */
  float conf_thresh;    /* 0.05 */
  float nms_thresh;     /* 0.5 */
  int32_t cross_class;  /* detection.py:111-135 variant */
  int32_t conf_ld;      /* floats between consecutive priors' class rows in `conf`; 0 = C (dense).  The engine pads the rows
                         * to a multiple of 4 (81 -> 84) so that the head GEMM / Winograd output transform can write them
                         * with 16-byte stores */
  int32_t _pad1;
  /* workspaces (caller-allocated) */
  float *scores_t;      /* [B,C-1,P] class-major foreground scores */
  int32_t *keep;        /* [B,P] 1 if max fg score > conf_thresh */
  int32_t *num_keep;    /* [B] K */
  float *maxsc;         /* [B,P] max foreground score per prior */
  int32_t *argmax;      /* [B,P] its class (0-based foreground index) */
  float *cand_score;    /* [B,(C-1)*top_k] per-class survivors, -1 where empty */
  int32_t *cand_prior;  /* [B,(C-1)*top_k] */
  /* outputs, fixed capacity cap = cross_class ? top_k : max_det */
  int32_t *out_count;   /* [B] */
  float *out_box;       /* [B,cap,4] x1,y1,x2,y2 relative */
  float *out_score;     /* [B,cap] */
  int64_t *out_class;   /* [B,cap] */
  float *out_coef;      /* [B,cap,D] */
  int32_t *out_prior;   /* [B,cap] index of the source prior (parity checks) */
  float *out_rec;       /* optional [B, 1 + cap*(6+D)]: the same detections as ONE fixed-size fp32 record per image — count, then per
                         * detection box 4 | score | class | coef D — i.e. the payload of the data-parallel gather
                         * (yolact_amd/parallel.py) written by the selection kernel itself; rows past the count are left untouched */
} ymi_detect_desc;
int ymi_detect_f32(const ymi_detect_desc *d, void *stream);

/* -- Detect with traditional NMS (ABI 9; csrc/detect_greedy.hip) ------------------------------------------------------------------
 * The reference's use_fast_nms = False mode (detection.py:80-108,182-228, utils/cython_nms.pyx): per class, every prior whose class
 * score is > conf_thresh is a candidate (no top_k cap); boxes are decoded and scaled by box_scale (cfg.max_size); candidates are
 * visited in descending score and a kept box suppresses every later one with overlap >= nms_thresh, overlap in pixels with the
 * "+1" convention of cython_nms.pyx; the survivors of all classes are sorted by score and cut to max_det.  Returned boxes are
 * (box * box_scale) / box_scale.  Ties (undefined in the reference): score desc, then class asc, then prior asc.
 * Reads from `d`: conf, loc, coef, priors, B, P, C, D, conf_ld, conf_is_logits, max_det (<= 256), conf_thresh, nms_thresh, scores_t
 * (workspace, [B,C-1,P]) and the outputs out_* (out_rec optional) with cap = max_det whatever `cross_class` says (the reference runs
 * per-class greedy NMS with use_cross_class_nms too); top_k, keep, num_keep, maxsc, argmax, cand_score and cand_prior are unused.
 * No host synchronisation, fixed launch shapes: graph-capturable. */
typedef struct {
  float box_scale;      /* cfg.max_size */
  int32_t _pad0;
  void *ws;             /* workspace of ymi_workspace_bytes(YMI_WS_DETECT_GREEDY, d) bytes, 16-byte aligned */
} ymi_detect_greedy_ws;
int ymi_detect_traditional_f32(const ymi_detect_desc *d, const ymi_detect_greedy_ws *g, void *stream);

/* -- postprocess: mask assembly (layers/output_utils.py:69-99, layers/box_utils.py:327-373) */
/* masks_lo[n,y,x] = crop(sigmoid(sum_k proto[y,x,k]*coef[n,k]), box[n]);  proto [ph,pw,D], coef [N,D], box [N,4] */
int ymi_lincomb_crop_f32(const float *proto, const float *coef, const float *box, float *masks_lo,
                         int ph, int pw, int D, int N, int crop, void *stream);
/* out[n,y,x] = bilinear(masks_lo[n], (h,w))[y,x] > thresh ? 1 : 0 (float32) ; thresh<0 -> no binarise */
int ymi_mask_upsample_f32(const float *masks_lo, float *out, int N, int ph, int pw, int h, int w,
                          float thresh, void *stream);
/* The same two steps for a whole fixed-capacity batch in ONE launch each (the per-image Python loop of eval.py:149 /
 * output_utils.py:35 collapsed): proto [B,ph,pw,D], coef [B,cap,D], box [B,cap,4], masks_lo [B,cap,ph,pw], out
 * [B,cap,h,w]; count [B] int32 ON THE DEVICE = live detections per image (null: all cap); rows past count[b] are
 * left untouched. */
int ymi_lincomb_crop_batch_f32(const float *proto, const float *coef, const float *box, const int32_t *count,
                               float *masks_lo, int B, int cap, int ph, int pw, int D, int crop, void *stream);
int ymi_mask_upsample_batch_f32(const float *masks_lo, const int32_t *count, float *out, int B, int cap, int ph, int pw,
                                int h, int w, float thresh, void *stream);
/* Which kernel the two upsample calls above run for these arguments (host only: no launch, no device access): one of YMI_UP_*, or
 * the YMI_E* code the call itself returns (YMI_ENULL out_addr 0, YMI_EARG a size <= 0 or nmask > 65535 with a count, YMI_ESHAPE a
 * count with a width only the flat kernel takes).  nmask = N, or B * cap; out_addr = the `out` pointer (its alignment takes part);
 * has_count != 0: ymi_mask_upsample_batch_f32 with a count, 0: without one, and ymi_mask_upsample_f32.  The launcher calls the
 * same function, and it respects the A/B switches YOLACT_AMD_UPSAMPLE / YOLACT_AMD_UPSAMPLE_FLAT (the latter: calls without a
 * count).  All four kernels write the same bits.  Additive to ABI 9. */
enum { YMI_UP_FLAT = 1, YMI_UP_BAND = 2, YMI_UP_ROWS16 = 3, YMI_UP_ROWS32 = 4 };
int ymi_mask_upsample_kernel(int nmask, int ph, int pw, int h, int w, uintptr_t out_addr, int has_count);
/* boxes [N,4] relative -> int64 absolute pixels via sanitize_coordinates(cast=False) then truncation */
int ymi_boxes_to_pixels(const float *box, int64_t *out, int N, int w, int h, void *stream);

/* -- FastBaseTransform (utils/augmentations.py:616-658): img [N,H,W,3] float32 BGR -> bilinear (align_corners=False)
 * resize to (oh, ow) -> normalisation -> RGB.  mean_bgr / std_bgr: HOST pointers to 3 floats in BGR order
 * (data/config.py:28-29).  mode: 0 (x-mean)/std, 1 x-mean, 2 x/255, 3 none (backbone.transform, data/config.py:181-202).
 * out_nhwc4 = 0: out [N,3,oh,ow] (the reference's return value); 1: out [N,oh,ow,4] RGB0 = the engine's input layout. */
int ymi_fast_base_transform_f32(const float *img, float *out, int N, int H, int W, int oh, int ow,
                                const float *mean_bgr, const float *std_bgr, int mode, int out_nhwc4, void *stream);

/* -- SSDAugmentation (utils/augmentations.py:667-688; csrc/augment.hip; additive, the ABI number stays) --------------------------------
 * The training transform's pixels for B images in two launches: one gather per output pixel of the S x S images, one per pixel of
 * every KEPT ground-truth mask.  Every random decision was made on the host (yolact_amd.utils.augmentations.draw_augmentation) and
 * arrives in one ymi_augment_rec per image; no canvas exists anywhere.  For output pixel (y, x):
 *   1. cv2.resize's INTER_LINEAR sample coordinate in the cropped image (ch, cw) = (crop_y1 - crop_y0, crop_x1 - crop_x0):
 *      f = (float)((x + 0.5) * ((double)cw / S) - 0.5), i = floor(f), f -= i; i < 0: i = 0, f = 0; i >= cw - 1: i = cw - 1, f = 0; the
 *      second tap is min(i + 1, cw - 1).  Rows likewise.
 *   2. each of the four taps: undo the mirror (cw - 1 - x), add the crop origin, subtract the expand offset.  Outside the source the
 *      tap is the fill colour mean_bgr, NOT distorted; inside it is the source pixel as float through the photometric chain.
 *   3. the chain, fp32, no clamping anywhere, a stage whose YMI_AUG_* bit is clear is SKIPPED: + delta; * alpha (unless
 *      CONTRAST_LAST); with YMI_AUG_PHOTOMETRIC the BGR -> HSV -> BGR round trip of OpenCV's float cvtColor, always: V = max,
 *      S = (V - min) / (|V| + FLT_EPSILON), H = (g - b | b - r | r - g) * (60 / (V - min + FLT_EPSILON)) + 0 | 120 | 240 by the
 *      channel that is the max (r first, then g), + 360 if negative; S *= sat; H += hue, then - 360 if above 360, then + 360 if below 0;
 *      back: h = H * (6 / 360), wrapped once into [0, 6), sector = floor(h), f = h - sector (a sector outside 0..5: sector 0, f 0),
 *      tab = {V, V(1 - S), V(1 - S f), V(1 - S(1 - f))}, (b, g, r) = tab[{1,3,0} | {1,0,2} | {3,0,1} | {0,2,1} | {0,1,3} | {2,1,0}];
 *      * alpha (with CONTRAST_LAST).
 *   4. bilinear in fp32, the horizontal pair first: (t00 (1 - fx) + t01 fx) (1 - fy) + (t10 (1 - fx) + t11 fx) fy; then mode (as
 *      ymi_fast_base_transform_f32: 0 (t - mean) / std, 1 t - mean, 2 t / 255, 3 none), BGR -> RGB, and out_nhwc4 as there:
 *      out [B,3,S,S], or [B,S,S,4] RGB0 (16-byte aligned: one store per pixel).  Image b of the table goes to slot out_slot.
 *   Masks: the same geometry, taps outside the source are 0, interpolated in integers as cv2's 8-bit path does: ax1 = rint(2048 fx),
 *   ax0 = 2048 - ax1, ay likewise, (ay0 (ax0 m00 + ax1 m01) + ay1 (ax0 m10 + ax1 m11) + 2^21) >> 22.  Output mask mask_first + j of
 *   image b is its instance kept[kept_first + j]; masks_out is [n_masks,S,S] float32, or uint8 with masks_u8.  Instances that are not
 *   listed are never read.
 * The table (records, one (image, instance) pair per output mask, each image's two resize scales as doubles, divided on the host: the
 * same IEEE quotient a pixel would compute) reaches the device in ONE copy into ws, enqueued on `stream`
 * from pageable host memory, so the caller's host arrays may be reused when the call returns.  No atomics; every output element is
 * written exactly once; the same inputs give the same bits.
 * YMI_ENULL: the descriptor, recs, out, ws, a record's src, kept / masks_out with n_masks > 0, a record's masks with n_kept > 0;
 * YMI_EARG: B, S < 1, n_masks < 0, mode outside 0..3, a source or canvas size < 1, an empty crop; YMI_ESHAPE: the expand offset
 * puts the source outside the canvas, the crop leaves the canvas, an instance index outside [0, n_inst), out_slot outside [0, B) or
 * used twice, the images' mask ranges not tiling [0, n_masks) exactly, ws_bytes too small, ws not 16-byte aligned, out not 16-byte aligned with out_nhwc4, S * S >= 2^31.  No error path launches or copies anything. */
enum { YMI_AUG_PHOTOMETRIC = 1, YMI_AUG_BRIGHTNESS = 2, YMI_AUG_CONTRAST = 4, YMI_AUG_CONTRAST_LAST = 8, YMI_AUG_SATURATION = 16,
       YMI_AUG_HUE = 32, YMI_AUG_MIRROR = 64, YMI_AUG_SRC_F32 = 128 };
typedef struct ymi_augment_rec {
  const void *src;              /* [h,w,3] BGR on the device: uint8, or float32 with YMI_AUG_SRC_F32 */
  const uint8_t *masks;         /* [n_inst,h,w] uint8 on the device (may be NULL when n_kept == 0) */
  int32_t h, w, n_inst, flags;  /* flags: YMI_AUG_* */
  int32_t canvas_h, canvas_w, off_x, off_y;          /* Expand's canvas and the source's corner in it (h, w, 0, 0 without one) */
  int32_t crop_x0, crop_y0, crop_x1, crop_y1;        /* RandomSampleCrop's rect in the canvas (0, 0, canvas_w, canvas_h without one) */
  float delta, alpha, sat, hue;
  int32_t out_slot, mask_first, n_kept, kept_first;  /* kept_first: this image's first entry of ymi_augment_desc.kept */
} ymi_augment_rec;
typedef struct ymi_augment_desc {
  const ymi_augment_rec *recs;  /* HOST [B] */
  const int32_t *kept;          /* HOST: the instance indices of every image's kept masks */
  float *out;                   /* [B,3,S,S] | [B,S,S,4] */
  void *masks_out;              /* [n_masks,S,S] float32 | uint8 */
  void *ws;                     /* DEVICE, ymi_workspace_bytes(YMI_WS_AUGMENT, desc) bytes, 16-byte aligned */
  int64_t ws_bytes;
  int32_t B, S, n_masks, mode, out_nhwc4, masks_u8;
  float mean_bgr[3], std_bgr[3];   /* the fill colour is mean_bgr in every mode */
} ymi_augment_desc;
int ymi_ssd_augment_f32(const ymi_augment_desc *d, void *stream);

/* -- mask_iou (layers/box_utils.py:98-113; consumer: eval.py:376-384,435-440 prep_metrics) --------------------------
 * masks_a [A,n], masks_b [B,n] float32 (n = h*w) -> iou [A,B] = inter / (area_a + area_b - inter), or inter / area_a when
 * iscrowd.  ws: caller-allocated workspace of A*B + A + B floats.  Exact for 0/1 masks (integer partial sums). */
int ymi_mask_iou_f32(const float *masks_a, const float *masks_b, int A, int B, long n, int iscrowd, float *ws, float *iou,
                     void *stream);

/* -- prep_metrics without float masks (eval.py:376-384,416-440; layers/box_utils.py:33-80,98-113) ------------------------ */
/* out[a,b] = IoU of point-form boxes a, b (iscrowd: intersection / area_a), reference op order.  box_a [A,4], box_b [B,4]. */
int ymi_jaccard_f32(const float *box_a, const float *box_b, int A, int B, int iscrowd, float *out, void *stream);
/* Masks as bits: word j of mask m (bits[m * W64 + j], W64 = ceil(n / 64)) holds pixels 64 j .. 64 j + 63 of the flat [h*w] mask
 * (bit i = pixel 64 j + i; padding bits 0).  ymi_mask_bits_f32 packs float masks [N, n] (bit = value > 0.5: ground truth);
 * ymi_mask_upsample_bits does F.interpolate(masks_lo [N,ph,pw], (h,w), bilinear) > thresh (output_utils.py:91-94) straight into
 * bits: every bit equals the pixel ymi_mask_upsample_f32 writes, 1/32 of the bytes. */
int ymi_mask_bits_f32(const float *masks, int N, long n, uint64_t *bits, void *stream);
int ymi_mask_upsample_bits(const float *masks_lo, int N, int ph, int pw, int h, int w, float thresh, uint64_t *bits, void *stream);
/* iou[a,b] from bit masks: popcount(a & b) / (|a| + |b| - popcount(a & b))  (iscrowd: / |a|) — integers below 2^24 evaluated in
 * fp32 exactly as box_utils.py:98-113 evaluates the float masks: bit-identical results. */
int ymi_mask_iou_bits(const uint64_t *bits_a, const uint64_t *bits_b, int A, int B, long W64, int iscrowd, float *iou, void *stream);

/* -- COCO box / mask AP (ABI 9, additive; csrc/ap_eval.hip) ---------------------------------------------------------------------
 * eval.py's metric mode on device: prep_metrics' matching (eval.py:445-510) per image, APDataObject.get_ap (eval.py:533-581) per
 * (type, threshold, class) at the end.  Types: 0 = box, 1 = mask; threshold k = (50 + 5 k) / 100, k < YMI_AP_NUM_THRESH.
 *
 * ymi_ap_match_f32: one image, one workgroup, no host synchronisation.  Inputs: N detections (classes int64, box / mask scores: the
 * same pointer for single-score models), IoU [N,G] against the non-crowd GT and crowd IoU (iscrowd) [N,Gc] for both types, GT and
 * crowd classes int32 (a class outside [0, num_classes) matches nothing; COCO crowds carry -1).  For each type t and each position
 * p of the type's order (box: stable by -box score; mask: the box order stably re-sorted by -mask score) it writes record
 * r = t * cap + base + p: rec_key = (class << 32) | 32-bit key ascending in -score (-0.0 == +0.0), rec_score = the type's score,
 * rec_flags = bit k: true positive at threshold k, bit 16 + k: pushed at threshold k (clear = matched a crowd region and dropped).
 * gt_count[c] += the image's non-crowd GT of class c.  N == 0 returns 0 without a launch: nothing is recorded, not even gt_count
 * (eval.py:405-406).  Limits: N <= YMI_AP_MAX_DET, G and Gc <= YMI_AP_MAX_GT, base + N <= cap.
 *
 * ymi_ap_finalize_f64: sorted_key [2,M] = rec_key[t, :M] stably sorted per row, perm [2,M] their positions in the row.  Writes
 * ap [2, YMI_AP_NUM_THRESH, num_classes] = get_ap() in fp64 (bit-equal to the reference) and empty [...] = is_empty(). */
#define YMI_AP_NUM_THRESH 10
#define YMI_AP_MAX_DET 1024
#define YMI_AP_MAX_GT 2048
typedef struct {
  const int64_t *cls;           /* [N] */
  const float *box_score;       /* [N] */
  const float *mask_score;      /* [N] */
  const float *box_iou;         /* [N,G] */
  const float *mask_iou;        /* [N,G] */
  const float *crowd_box_iou;   /* [N,Gc] */
  const float *crowd_mask_iou;  /* [N,Gc] */
  const int32_t *gt_cls;        /* [G] */
  const int32_t *crowd_cls;     /* [Gc] */
  int64_t *rec_key;             /* [2,cap] */
  float *rec_score;             /* [2,cap] */
  int32_t *rec_flags;           /* [2,cap] */
  int64_t *gt_count;            /* [num_classes], accumulated */
  int64_t base, cap;
  int32_t N, G, Gc, num_classes;
} ymi_ap_match_desc;
typedef struct {
  const int64_t *sorted_key;    /* [2,M] */
  const int64_t *perm;          /* [2,M] */
  const int32_t *rec_flags;     /* [2,cap] */
  const int64_t *gt_count;      /* [num_classes] */
  double *ap;                   /* [2,YMI_AP_NUM_THRESH,num_classes] */
  int32_t *empty;               /* [2,YMI_AP_NUM_THRESH,num_classes] */
  int64_t M, cap;
  int32_t num_classes, _pad0;
} ymi_ap_finalize_desc;
int ymi_ap_match_f32(const ymi_ap_match_desc *d, void *stream);
int ymi_ap_finalize_f64(const ymi_ap_finalize_desc *d, void *stream);

/* -- prep_display, GPU half (eval.py:186-209,228): alpha-composite n instance masks onto a frame.
 * img [h,w,3] float32 0..255 (channel order as given), masks [n,h,w] float32, colors [n,3] float32 0..1 (device, same
 * channel order as img), out [h,w,3] uint8.  n = 0 just converts the frame. */
int ymi_composite_masks_u8(const float *img, const float *masks, const float *colors, int n, int h, int w, float alpha,
                           unsigned char *out, void *stream);

/* -- COCO result wire format (eval.py:320-324 Detections.add_mask -> pycocotools.mask.encode; maskApi.c rleEncode,
 * rleToString): run lengths of the COLUMN-major flattening of each mask, starting with a (possibly empty) run of zeros.
 * masks [N,h,w] float32 (nonzero = foreground; the path's masks are exactly {0,1}), w <= 2048.
 * counts [N,cap] uint32, nruns [N] = true number of runs of each mask (a mask with nruns > cap was truncated: retry
 * with a larger cap). */
int ymi_mask_rle_f32(const float *masks, int N, int h, int w, uint32_t *counts, int32_t *nruns, int cap, void *stream);
/* The same counts for the masks `ymi_mask_upsample_f32(masks_lo, ..., thresh)` WOULD write, without writing them: upsample
 * (bilinear, align_corners=False, output_utils.py:91), threshold (`> thresh`, :94) and run-length encoding in one kernel.
 * masks_lo [N,ph,pw] = the cropped sigmoid masks at prototype resolution (ymi_lincomb_crop_f32).  The COCO result path
 * (eval.py:403-429) then reads N*ph*pw*4 bytes instead of writing and re-reading N*h*w*4.  32*w + 12*h <= 65536 (LDS tables). */
int ymi_mask_rle_upsampled_f32(const float *masks_lo, int N, int ph, int pw, int h, int w, float thresh, uint32_t *counts,
                               int32_t *nruns, int cap, void *stream);
/* counts -> the ASCII string pycocotools stores in 'counts' (delta to counts[i-2] for i > 2, 5 bits per character,
 * 0x20 = continuation, + 48).  str [N,cap_chars] bytes, nchars [N] = true length (> cap_chars: truncated). */
int ymi_rle_to_string(const uint32_t *counts, const int32_t *nruns, int N, int cap, uint8_t *str, int32_t *nchars,
                      int cap_chars, void *stream);

/* -- COCODetection.pull_item's image read (data/coco.py:138-141: `img = cv2.imread(path)` -> uint8 BGR [h,w,3]) ----------
 * cv2.imread on a JPEG = libjpeg-turbo with the library defaults (ISLOW IDCT, fancy upsampling) + EXIF orientation.
 * Split: the serial half (markers + Huffman decoding, baseline and progressive) runs on the HOST and yields the quantised
 * coefficient blocks; dequantisation, IDCT, chroma upsampling, YCbCr -> BGR and the orientation run on the GPU.
 * Bit-exact against libjpeg-turbo (pinned through oracle/jpeg_oracle.py).  Errors: YMI_EFORMAT corrupt / truncated
 * stream, YMI_EUNSUPPORTED a valid file outside this subset (arithmetic coding, lossless, 12-bit, CMYK / YCCK,
 * fractional sampling ratios). */
enum { YMI_JPEG_YCBCR = 0, YMI_JPEG_RGB = 1, YMI_JPEG_GRAY = 2 };
typedef struct {
  int32_t width, height;          /* as stored in the file (before the EXIF orientation is applied) */
  int32_t ncomp;                  /* 1 or 3 */
  int32_t progressive;
  int32_t orientation;            /* EXIF tag 0x0112, 1..8 (1 when absent) */
  int32_t color;                  /* YMI_JPEG_* : how the components map to BGR */
  int32_t out_width, out_height;  /* of the decoded image = (height, width) swapped for orientations 5..8 */
  int32_t hs[3], vs[3];           /* sampling factors as declared */
  int32_t hf[3], vf[3];           /* upsampling factors max_h / h, max_v / v */
  int32_t bw[3], bh[3];           /* block grid of each component, padded to whole MCUs */
  int32_t dw[3], dh[3];           /* real (downsampled) size of each component in samples */
  int64_t coef_count;             /* int16 coefficients in total = sum bw*bh*64 */
  int64_t plane_bytes;            /* device workspace for ymi_jpeg_reconstruct_bgr_u8 (uint8 planes) */
} ymi_jpeg_info;
/* HOST.  Header only: sizes for the caller's allocations. */
int ymi_jpeg_parse(const uint8_t *data, size_t n, ymi_jpeg_info *info);
/* HOST.  Entropy-decode every scan into coefs (host memory, coef_capacity int16; layout [component][by][bx][64], natural
 * (row-major) order inside a block, zero where no scan wrote) and latch the quantisation tables: qt [3][64] natural order. */
int ymi_jpeg_decode_coefs(const uint8_t *data, size_t n, int16_t *coefs, int64_t coef_capacity, uint16_t *qt,
                          ymi_jpeg_info *info);
/* DEVICE.  coefs / qt: device copies of the host results; planes_ws: info->plane_bytes; out: [out_height,out_width,3] uint8 BGR. */
int ymi_jpeg_reconstruct_bgr_u8(const ymi_jpeg_info *info, const int16_t *coefs, const uint16_t *qt, uint8_t *planes_ws,
                                uint8_t *out, void *stream);

/* -- the image write of evalimage / evalimages / evalvideo (eval.py: `cv2.imwrite(save_path, img_numpy)`) ------------------
 * cv2.imwrite of a .jpg = libjpeg with its defaults at quality 95: baseline sequential (SOF0), one interleaved scan, JFIF APP0,
 * the T.81 Annex K quantisation tables scaled by the quality, the four Annex K Huffman tables, YCbCr 4:2:0, ISLOW forward DCT.
 * Marker order SOI, APP0, DQT, DQT, SOF0, DHT x 4, SOS, data, EOI.  Here the whole encoder runs on the GPU (colour conversion,
 * edge padding, chroma downsampling, FDCT, quantisation, Huffman coding, byte stuffing: csrc/jpeg_enc.hip); the host writes
 * only the fixed-size header.  The stream is BYTE-EQUAL to libjpeg-turbo's through Pillow (`Image.save(.., 'JPEG', quality=q,
 * subsampling=2 or 0)`; tests/test_jpeg_encode.py, tests/test_gpu_jpeg_encode.py); cv2 calls the same library with the same
 * defaults but is not available to check against.
 *   file = [ymi_jpeg_write_header bytes] + [out[0 .. *out_len) of ymi_jpeg_encode_bgr_u8]       (the EOI marker is in `out`)
 * No host synchronisation, no device allocation, everything on `stream`. */
enum { YMI_JPEG_SUB_444 = 0, YMI_JPEG_SUB_420 = 2 };      /* Pillow's `subsampling` numbering; 4:2:0 is libjpeg's default */
#define YMI_JPEG_HEADER_BYTES 623
typedef struct ymi_jpeg_enc_desc {
  const uint8_t *img;    /* device, uint8 BGR [h,w,3] (display.prep_display's frame, ymi_jpeg_reconstruct_bgr_u8's output) */
  int32_t h, w;          /* 1..65535 each */
  int64_t row_stride;    /* bytes between rows, >= 3 * w; pixels inside a row are packed */
  int32_t quality;       /* 1..100 (cv2.imwrite's default: 95) */
  int32_t subsampling;   /* YMI_JPEG_SUB_420 / YMI_JPEG_SUB_444 */
  uint8_t *out;          /* device: entropy-coded scan (byte-stuffed, padded with 1-bits) followed by the EOI marker */
  int64_t out_capacity;  /* bytes at `out`, >= ymi_workspace_bytes(YMI_WS_JPEG_ENC_OUT, desc) (YMI_EARG otherwise) */
  int64_t *out_len;      /* device: bytes written to `out` */
  void *ws;              /* device workspace of ymi_workspace_bytes(YMI_WS_JPEG_ENC, desc) bytes, 256-byte aligned */
} ymi_jpeg_enc_desc;
/* HOST.  SOI .. SOS (YMI_JPEG_HEADER_BYTES bytes) into out [cap]; *n = bytes written.  YMI_EARG: h / w outside 1..65535,
 * quality outside 1..100, unknown subsampling, cap too small. */
int ymi_jpeg_write_header(int h, int w, int quality, int subsampling, uint8_t *out, size_t cap, size_t *n);
/* HOST.  The two quantisation tables header and kernels both use: qt [2][64] (luminance, chrominance), natural order. */
int ymi_jpeg_enc_qtables(int quality, uint16_t *qt);
/* DEVICE.  YMI_EARG: the cases of ymi_jpeg_write_header, row_stride < 3 * w, out_capacity below the bound; YMI_ENULL: a
 * null img / out / out_len / ws. */
int ymi_jpeg_encode_bgr_u8(const ymi_jpeg_enc_desc *d, void *stream);

/* -- COCODetection.pull_item's ground-truth masks (data/coco.py:144-148: `self.coco.annToMask(obj)`), HOST code -----------
 * pycocotools maskApi.c restated (pycocotools is an unpinned pip dependency of the reference, environment.yml:30):
 * rleFrPoly / rleFrString / rleDecode.  Every call ORs its region into mask [h,w] uint8 ROW-major (0/1), so a polygon
 * list (union of polygons, rleMerge intersect = 0) is a loop of calls on one zeroed mask. */
int ymi_coco_poly_fill_u8(const double *xy, int k, int h, int w, uint8_t *mask);          /* k vertices, x0 y0 x1 y1 ... */
int ymi_coco_rle_fill_u8(const uint32_t *counts, long n, int h, int w, uint8_t *mask);    /* uncompressed counts */
int ymi_coco_rle_string_fill_u8(const char *s, long len, int h, int w, uint8_t *mask);    /* compressed 'counts' string */
/* HOST.  rleFrString alone: the compressed string's counts (at most len of them) into counts[cap]; returns how many, or
 * YMI_ENULL / YMI_EARG (len, cap < 0, cap too small) / YMI_EFORMAT (what ymi_coco_rle_string_fill_u8 returns for the string). */
int64_t ymi_coco_rle_string_counts(const char *s, long len, uint32_t *counts, int64_t cap);

/* -- the same masks rasterised on the DEVICE (csrc/coco_mask.hip): all annotations of one image, or of a batch of images with
 * their own h, w, in ONE call and ONE upload.  Record i writes out [h,w] uint8 ROW-major, every byte 0 or 1 (nothing is
 * OR-ed: the caller zeroes nothing), byte-equal to ymi_coco_poly_fill_u8 looped over the record's polygons
 * (YMI_COCO_POLY) or to ymi_coco_rle_fill_u8 (YMI_COCO_COUNTS; a compressed string goes through
 * ymi_coco_rle_string_counts first) on a zeroed mask.
 *   One workgroup per record.  Polygon: every point of the 5x upsampled boundary walk is recomputed from its edge in fp64
 *   with the host's operations in the host's order ((int)(5 v + .5), s = (double)(ye - ys) / dx, (int)(ys + s t + .5),
 *   (xd + .5) / 5 - .5, floor / clamp / ceil; no contraction, IEEE division), compared with its predecessor (an edge's
 *   first point: the previous edge's last), and a qualifying crossing toggles bit x h + y of a COLUMN-major bitmap of
 *   h w + 1 bits in LDS (integer atomic XOR: commutative, so the bits do not depend on the order).  A prefix XOR over the
 *   whole bitmap, carried across column ends as the host's sorted run lengths carry it, is the polygon; it is OR-ed into the
 *   record's union bitmap.  Counts: the prefix sums of the counts are the toggled bits, then the same prefix XOR.  Last, the
 *   union bitmap is transposed into the row-major bytes with 4-byte stores (single bytes up to out's alignment and at the end).
 * LIMIT: the two bitmaps of a record must fit the 160 KiB of LDS a gfx950 workgroup may declare:
 * h * w <= YMI_COCO_MASK_MAX_PIXELS = 640000 (800 x 800), otherwise YMI_EUNSUPPORTED (rasterise that annotation on the host).
 * Validated on the host before anything is copied or launched, with the host codec's rules and codes -- the kernel reports
 * nothing.  YMI_ENULL: the descriptor, recs, ws, a record's out, xy / poly_len with a polygon record, counts with a counts
 * record; YMI_EARG: n < 1, a record's h, w <= 0, an unknown kind, n < 0 (a polygon record without polygons is the empty mask), a polygon
 * of < 1 vertices, a coordinate that is NaN or |c| > 3 max(w, h) + 1024; YMI_EFORMAT: a run past h w, counts that do not sum to
 * h w; YMI_ESHAPE: a record's range outside its table (n_vert, n_poly, n_counts), ws_bytes too small, ws not 16-byte
 * aligned; YMI_EUNSUPPORTED: above.  The table (vertices, records, polygon lengths, counts) reaches the device in one copy
 * into ws from pageable host memory, enqueued on `stream`: the caller's arrays may be reused when the call returns. */
#define YMI_COCO_MASK_MAX_PIXELS 640000
enum { YMI_COCO_POLY = 0, YMI_COCO_COUNTS = 1 };
typedef struct ymi_coco_mask_rec {
  uint8_t *out;             /* DEVICE [h,w] */
  int32_t kind, h, w, n;    /* n: polygons (YMI_COCO_POLY) | counts (YMI_COCO_COUNTS) */
  int32_t first;            /* POLY: the record's first entry of poly_len; COUNTS: its first entry of counts */
  int32_t xy_first;         /* POLY: its first VERTEX of xy (the polygons' vertices follow one another) */
} ymi_coco_mask_rec;
typedef struct ymi_coco_mask_desc {
  const ymi_coco_mask_rec *recs;  /* HOST [n] */
  const double *xy;               /* HOST [n_vert,2]: x0 y0 x1 y1 ... of every polygon of every record */
  const int32_t *poly_len;        /* HOST [n_poly]: vertices of each polygon */
  const uint32_t *counts;         /* HOST [n_counts] */
  void *ws;                       /* DEVICE, ymi_workspace_bytes(YMI_WS_COCO_MASK, desc) bytes, 16-byte aligned */
  int64_t ws_bytes;
  int64_t n_vert, n_poly, n_counts;
  int32_t n, _pad0;
} ymi_coco_mask_desc;
int ymi_coco_masks_u8(const ymi_coco_mask_desc *d, void *stream);

/* -- DCNv2 forward (external/DCNv2/src/vision.cpp:5, dcn_v2.h:9-39, dcn_v2_cuda.cu:42-172) ---- */
typedef struct {
  ymi_conv_desc conv;    /* main 3x3 conv: x, packed w, bias, epilogue, outputs (kh=kw=3, pad=1) */
  const float *offmask;  /* [B,Ho,Wo,ldo] NHWC output of conv_offset_mask: ch 2k=dh_k, 2k+1=dw_k, 18+k=mask logit (om_layout 0) */
  int32_t ldo;           /* channel stride of offmask pixels (>= 27) */
  int32_t mask_is_prob;  /* 0: channels 18.. are mask LOGITS, the kernel applies the sigmoid (DCN.forward, dcn_v2.py:118-128 — the
                          * engine's plans); 1: they are the modulation itself, already in [0,1] (dcn_v2_conv / DCNv2.forward,
                          * dcn_v2.py:16-33,85-96, whose callers pass torch.sigmoid(mask)).  Occupies what was tail padding. */
  int32_t om_layout;     /* channel order of offmask.  0: the reference's (dcn_v2.py:118-122: 18 offsets, then 9 masks).  1: per tap
                          * [dh_k, dw_k, mask_k] at channels 3k .. 3k+2 — a caller that owns conv_offset_mask's filters (the engine)
                          * permutes their ROWS once on the host, and the gather kernel then fetches a tap's three values with one
                          * 12-byte load instead of three (it is bound by vector-memory instructions) */
  int32_t _pad1;
} ymi_dcn_desc;
int ymi_dcn_v2_forward_f32(const ymi_dcn_desc *d, void *stream);

/* -- DCNv2 backward (dcn_v2.py:35-52, dcn_v2_cuda.cu:174-335, dcn_v2_im2col_cuda.cu:197-327; csrc/dcn_bwd.hip; additive at ABI 9) --
 * Gradients of y = ymi_dcn_v2_forward_f32(x, offmask, w, bias) for the geometry the forward takes: 3x3, pad 1, dilation 1, one
 * deformable group, square stride 1 or 2, Cin % 32 == 0 (the caller pads with zero channels), mask_is_prob = 1 (channels 18.. of
 * offmask ARE the modulation; a caller that holds logits applies the sigmoid and its derivative itself).  Everything is fp32 NHWC.
 * One pointer per gradient; NULL = not wanted, and its work is skipped (all NULL: no launch).  The call zeroes what it
 * accumulates into, so outputs need no initialisation.  No workspace: neither the column tensor nor its gradient is
 * materialised.  gx, gw, gbias (and g_offset / g_mask on small maps) are sums of fp32 atomics: fp32-class accurate, NOT
 * bit-reproducible from run to run.  YMI_EARG: kernel / pad / dilation / groups / stride / mask_is_prob / om_layout outside the
 * above; YMI_ESHAPE: Cin % 32, ldx < Cin or ldx % 4, ldo < 27, Ho / Wo not the convolution's output size, a tensor of 2^31
 * elements or more, x / gy / gx not 16-byte aligned; YMI_ENULL: a needed input is NULL.  No error path launches anything. */
typedef struct ymi_dcn_bwd_desc {
  const float *x;        /* [B,H,W,ldx] the forward's input */
  const float *offmask;  /* [B,Ho,Wo,ldo] the forward's offsets and modulation, ldo / om_layout as in ymi_dcn_desc */
  const float *w;        /* fp32 filters [Cout][3][3][Cin] (UNPACKED: k = (3i + j) * Cin + c); may be NULL when only gw / gbias are wanted */
  const float *gy;       /* [B,Ho,Wo,Cout] dense: gradient of the output */
  float *gx;             /* [B,H,W,ldx] (channels >= Cin are zeroed) */
  float *g_offset;       /* [B,Ho,Wo,18] dense: channel 2k = d/d dh_k, 2k+1 = d/d dw_k (whatever om_layout the input has) */
  float *g_mask;         /* [B,Ho,Wo,9] dense: d/d mu_k */
  float *gw;             /* [Cout][3][3][Cin], the layout of w */
  float *gbias;          /* [Cout] */
  int32_t B, H, W, Cin, ldx, Ho, Wo, Cout;
  int32_t kh, kw, stride, pad, dilation, deformable_groups;
  int32_t ldo, mask_is_prob, om_layout, _pad0;
} ymi_dcn_bwd_desc;
int ymi_dcn_v2_backward_f32(const ymi_dcn_bwd_desc *d, void *stream);

/* -- the train path's deformable convolution: the column tensor and its backward (csrc/dcn_train.hip; additive at ABI 9) -----------
 * The im2col half of DCNv2 (dcn_v2_im2col_cuda.cu:143-327) for the same geometry — 3x3, pad 1, dilation 1, one deformable group,
 * square stride 1 or 2, Cin % 32 == 0 — on dense NHWC fp32, with om [B,Ho,Wo,27] the RAW output of conv_offset_mask: channel 2k =
 * dh_k, 2k + 1 = dw_k, 18 + k = the mask LOGIT of tap k = 3i + j (the sigmoid and its derivative are applied here).  The GEMM half is
 * ymi_conv2d_nhwc_f32 / ymi_conv_wgrad_nhwc_f32 on col as a 1x1 convolution of 9 Cin channels.  item = m * 9 + k, m = (b, oy, ox).
 *   ymi_dcn_cols_fwd_f32      col[item, c] = sigmoid(logit_k) * bilinear(x, point_k)[c], zero-padded, 0 for a point outside
 *                             -1 < h < H, -1 < w < W (the point formed in fp32 as ymi_dcn_v2_forward_f32 forms it).  Reads x, om.
 *   ymi_dcn_cols_entries_f32  the inverted index's raw material: entry e = item * 4 + corner (top-left, top-right, bottom-left,
 *                             bottom-right) gets keys[e] = the corner's pixel (b*H + y)*W + x, or B*H*W when the corner is outside the
 *                             image or the point is gated out, and coef[e] = corner weight * mu (0 there).  Reads om.
 *   ymi_dcn_cols_bwd_f32      from dcol [B,Ho,Wo,9*Cin]: g_om [B,Ho,Wo,27] (d/d dh_k, d/d dw_k, d/d logit_k; exactly 0 for a gated-out
 *                             point; at an integer coordinate the derivative of the cell [h, h + 1]) and gx [B,H,W,Cin].  Either may
 *                             be NULL (both: no launch).  gx needs sorted_keys / order — keys sorted ascending by a STABLE sort and
 *                             the permutation that did it (order[i] = the entry at sorted position i) — coef as written above, and
 *                             seg, B*H*W + 1 ints of scratch.  g_om needs x and om.
 * SUMMATION ORDER (part of the contract, a function of the shape and of om only): a dot product over channels — lane l of eight
 * adds the channels 4 l + 32 j + e, j ascending, e = 0 .. 3, from +0.0, then the lanes combine by the butterfly 4, 2, 1; gx[t, c] —
 * from +0.0, (coef[e] * dcol[e / 4, c]) over the entries of pixel t in ascending e.  No floating-point atomics: the same inputs
 * give the same bits.  Every element of every output is written.  An order[] value outside [0, 36 B Ho Wo) is skipped, a run
 * outside the list is clipped: a wrong permutation gives wrong sums, never an access outside the tensors.
 * YMI_EARG: a size < 1, stride not 1 / 2; YMI_ESHAPE: Cin % 32, Ho / Wo not the convolution's output size, x, col, dcol, om or the
 * entry list (36 B Ho Wo) of 2^31 elements or more, x / col / dcol / gx / keys / coef not 16-byte aligned; YMI_ENULL: a pointer the
 * call needs is NULL.  No error path launches anything. */
typedef struct ymi_dcn_cols_desc {
  const float *x;               /* [B,H,W,Cin] */
  const float *om;              /* [B,Ho,Wo,27] */
  float *col;                   /* [B,Ho,Wo,9*Cin] (fwd: written) */
  const float *dcol;            /* [B,Ho,Wo,9*Cin] (bwd: read) */
  float *g_om;                  /* [B,Ho,Wo,27] or NULL */
  float *gx;                    /* [B,H,W,Cin] or NULL */
  int32_t *keys;                /* [36 B Ho Wo] (entries: written) */
  float *coef;                  /* [36 B Ho Wo] (entries: written; bwd: read) */
  const int32_t *sorted_keys;   /* [36 B Ho Wo] (bwd, gx) */
  const int64_t *order;         /* [36 B Ho Wo] (bwd, gx) */
  int32_t *seg;                 /* [B*H*W + 1] scratch (bwd, gx) */
  int32_t B, H, W, Cin, Ho, Wo, stride, _pad0;
} ymi_dcn_cols_desc;
int ymi_dcn_cols_fwd_f32(const ymi_dcn_cols_desc *d, void *stream);
int ymi_dcn_cols_entries_f32(const ymi_dcn_cols_desc *d, void *stream);
int ymi_dcn_cols_bwd_f32(const ymi_dcn_cols_desc *d, void *stream);

/* -- lincomb mask loss 'M' with gradients (layers/modules/multibox_loss.py:499-627,650; csrc/mask_loss.hip; additive at ABI 9) --
 * The mask term of MultiBoxLoss for the switches both shipped base configs train with (mask_proto_crop,
 * mask_proto_normalize_emulate_roi_pooling, binarised downsampled GT, sigmoid), for a whole batch in one call:
 *     x = sum_k proto[b,r,c,k] coef[j,k],  p = sigmoid(x),  q = inside_j(r,c) ? p : 0        (crop window: box_utils.py:328-373, padding 1)
 *     l = -(t max(log q, -100) + (1 - t) max(log(1 - q), -100)),  L_j = sum_{r,c} l
 *     roi_norm: L_j = L_j / ((b2 - b0) mw) / ((b3 - b1) mh) * (crop ? mh mw : 1)
 *     loss = alpha / mh / mw * sum_j weight_j L_j
 * and, where asked, d loss / d proto and d loss / d coef (dl/dx = inside ? p - t : 0) from the same pass: no tensor of mh*mw*N
 * elements exists.  Every element of every output is written by the call (zeros for images without instances); N = 0 is legal
 * (loss 0, d_proto 0).  No floating-point atomics: the same inputs give the same bits.  For |x| > ~17, where the reference's fp32
 * sigmoid saturates, l = min(softplus, 100) and dl/dx = p - t (finite).
 * YMI_ESHAPE: K != 32, mh*mw >= 2^26, N >= 2^24, proto / d_proto / ws not 16-byte aligned; YMI_EARG: B outside 1..65535, mh / mw < 1,
 * N < 0, G < 1 with N > 0, crop / roi_norm not 0 / 1; YMI_ENULL: proto, img_off or loss NULL, or (N > 0) coef, box, gt, gt_idx,
 * weight or ws NULL.  No error path launches anything. */
typedef struct ymi_mask_loss_desc {
  const float *proto;      /* [B,mh,mw,K] NHWC, the protonet's output layout */
  const float *coef;       /* [N,K] coefficient rows of the positives, image by image */
  const float *box;        /* [N,4] relative point form (x1, y1, x2, y2): the rows of gt_box_t */
  const uint8_t *gt;       /* [G,mh,mw] 0 / non-zero: the downsampled, binarised GT masks of the batch */
  const int32_t *gt_idx;   /* [N] row of gt of each instance (clamped to 0..G-1) */
  const int32_t *img_off;  /* [B+1] instances of image b are [img_off[b], img_off[b+1]).  PRECONDITION (device data, not checked):
                            * img_off[0] = 0, img_off[B] = N, non-decreasing — an instance no image covers has no partial sums, and
                            * loss, loss_inst and d_coef would then be summed from unwritten workspace (no access is out of bounds) */
  const float *weight;     /* [N] old_num_pos / num_pos of the instance's image (multibox_loss.py:624-625) */
  float *loss;             /* [1] */
  float *loss_inst;        /* [N] L_j (after roi_norm, before weight); may be NULL */
  float *d_proto;          /* [B,mh,mw,K]; may be NULL */
  float *d_coef;           /* [N,K]; may be NULL */
  void *ws;                /* ymi_workspace_bytes(YMI_WS_MASK_LOSS, desc) bytes, 16-byte aligned */
  int32_t B, mh, mw, K, N, G;
  int32_t crop, roi_norm;  /* 0 / 1: cfg.mask_proto_crop, cfg.mask_proto_normalize_emulate_roi_pooling */
  float alpha;             /* cfg.mask_alpha */
  int32_t _pad0;
} ymi_mask_loss_desc;
int ymi_mask_loss_f32(const ymi_mask_loss_desc *d, void *stream);

/* -- MultiBoxLoss target assignment and the box loss 'B' (layers/box_utils.py:159-265 match / encode, layers/modules/
 * multibox_loss.py:84-145; csrc/match.hip; additive at ABI 9) ------------------------------------------------------------------
 * For use_prediction_matching = use_change_matching = use_yolo_regressors = False, a whole batch in one call and four launches:
 * every prior takes the GT of the largest jaccard overlap (fp32, the reference's operation order, no FMA contraction, IEEE
 * division: the bits of torch's CPU jaccard), then the reference's greedy loop forces each GT onto its best free prior
 * (overlap 2), then conf = label + 1, -1 below pos_thresh, 0 below neg_thresh, -1 for a non-positive whose crowd ratio
 * inter / area(prior) exceeds crowd_thresh (skipped for images without crowds and for crowd_thresh >= 1).  Every arg-max keeps
 * the LOWEST index among equal values.  Thresholds are compared in fp32.  loc_t = encode(gt_box_t, priors), variances 0.1 / 0.2.
 * With loc_data: loss = bbox_alpha * sum over positives of smooth_l1(loc_data - loc_t) (beta 1), and d_loc = bbox_alpha *
 * clamp(loc_data - loc_t, -1, 1) at positives, +0.0f elsewhere.  No atomics: the same inputs give the same bits.
 * The offsets are given twice: on the device for the kernels and on the host for this function, which checks the host copy (the
 * kernels clamp what they read, so that a device copy that differs cannot make an access out of bounds).
 * YMI_EARG: B outside 1..65535, P < 1, G < 1, Gc < 0, offsets that do not start at 0, end at G (Gc) or decrease, an image with
 * no GT or with more GTs than P, d_loc or loss without loc_data; YMI_ESHAPE: P, G or Gc >= 2^24, priors / truth / crowd /
 * loc_data / loc_t / gt_box_t / d_loc / ws not 16-byte aligned; YMI_ENULL: a required pointer NULL (crowd, crowd_off and
 * crowd_off_host only with Gc > 0).  No error path launches anything. */
typedef struct ymi_match_desc {
  const float *priors;            /* [P,4] centre-size form (cx, cy, w, h) */
  const float *truth;             /* [G,4] point form, the batch's non-crowd GT boxes image by image */
  const int32_t *label;           /* [G] class of each GT (conf_t = label + 1) */
  const int32_t *gt_off;          /* DEVICE [B+1]: the GTs of image b are [gt_off[b], gt_off[b+1]) */
  const int32_t *gt_off_host;     /* HOST   [B+1]: the same values */
  const float *crowd;             /* [Gc,4] point form crowd boxes; NULL when Gc = 0 */
  const int32_t *crowd_off;       /* DEVICE [B+1]; NULL when Gc = 0 */
  const int32_t *crowd_off_host;  /* HOST   [B+1]; NULL when Gc = 0 */
  const float *loc_data;          /* [B,P,4] predicted regressions; may be NULL (no loss, no d_loc) */
  float *loc_t;                   /* [B,P,4] */
  float *gt_box_t;                /* [B,P,4] truth[idx_t] */
  int32_t *conf_t;                /* [B,P] class + 1, 0 background, -1 neutral */
  int32_t *idx_t;                 /* [B,P] matched GT, counted within the image */
  uint8_t *pos;                   /* [B,P] conf_t > 0 */
  int32_t *num_pos;               /* [B] */
  float *d_loc;                   /* [B,P,4]; may be NULL */
  float *loss;                    /* [1]; may be NULL */
  void *ws;                       /* ymi_workspace_bytes(YMI_WS_MATCH, desc) bytes, 16-byte aligned */
  int32_t B, P, G, Gc;
  float pos_thresh, neg_thresh, crowd_thresh, bbox_alpha;
} ymi_match_desc;
int ymi_match_f32(const ymi_match_desc *d, void *stream);
/* The box loss of given targets: loc_data, loc_t [B,P,4], pos [B,P] 0 / non-zero -> loss [1] and (may be NULL) d_loc [B,P,4], the
 * loss half of ymi_match_f32 with the same partial sums, hence the same bits.  ws: ymi_workspace_bytes(YMI_WS_BOX_LOSS, desc)
 * bytes for a ymi_match_desc with B and P set.  Errors as above. */
int ymi_box_loss_f32(const float *loc_data, const float *loc_t, const uint8_t *pos, int B, int P, float bbox_alpha, float *loss,
                     float *d_loc, void *ws, void *stream);

/* -- the class loss 'C' with online hard example mining (layers/modules/multibox_loss.py:242-296 ohem_conf_loss, for
 * ohem_use_most_confident = use_class_balanced_conf = False; csrc/class_loss.hip; additive at ABI 9) ---------------------------
 * A whole batch in one call and four launches, loss and gradient together:
 *     lse = logsumexp(conf[b,i,:]) with the ROW's own maximum subtracted (the reference subtracts the batch's maximum, which is
 *           the same function but underflows to log 0 for a row far below it)
 *     key = lse - conf[b,i,0] for conf_t == 0, and 0 for positives (conf_t > 0) and neutrals (conf_t < 0)
 *     n_b = min(negpos_ratio * num_pos_b, P - 1); the n_b largest keys of image b are marked, EQUAL KEYS IN PRIOR ORDER (the lowest
 *           index wins; the reference's unstable sort leaves ties undefined); neg = marked and conf_t == 0 - a marked positive or
 *           neutral is dropped and not replaced (:261-265)
 *     loss = conf_alpha * sum over pos | neg of (lse - conf[b,i,conf_t])
 *     d_conf = conf_alpha * (softmax(conf[b,i,:]) - onehot(conf_t)) on the rows of pos | neg, +0.0f on every other row
 * The selection carries no gradient.  Every element of every output is written by the call.  No floating-point atomics: the same
 * inputs give the same bits.  A conf_t outside -1 .. C-1 is compared before it indexes: it reads nothing and makes loss NaN.
 * YMI_EARG: B outside 1..65535, P < 2, C outside 2..256, negpos_ratio < 0; YMI_ESHAPE: B*P*C >= 2^31, conf / d_conf / ws not
 * 16-byte aligned; YMI_ENULL: conf, conf_t, loss, neg, num_neg or ws NULL.  No error path launches anything. */
typedef struct ymi_class_loss_desc {
  const float *conf;       /* [B,P,C] logits */
  const int32_t *conf_t;   /* [B,P] class + 1, 0 background, -1 neutral (ymi_match_desc.conf_t) */
  float *loss;             /* [1] */
  uint8_t *neg;            /* [B,P] 0 / 1: the mined negatives */
  int32_t *num_neg;        /* [B] */
  float *d_conf;           /* [B,P,C]; may be NULL */
  void *ws;                /* ymi_workspace_bytes(YMI_WS_CLASS_LOSS, desc) bytes, 16-byte aligned */
  int32_t B, P, C;
  int32_t negpos_ratio;    /* MultiBoxLoss's negpos_ratio (3) */
  float conf_alpha;        /* cfg.conf_alpha */
  int32_t _pad0;
} ymi_class_loss_desc;
int ymi_class_loss_f32(const ymi_class_loss_desc *d, void *stream);

/* -- the semantic segmentation loss 'S' (layers/modules/multibox_loss.py:218-239; csrc/segm_loss.hip; additive at ABI 9) -------
 * A whole batch in one call and two launches: the target of channel c at a pixel is the OR of the image's GT masks whose label is
 * c (no target tensor exists: a thread keeps its pixel's K <= 128 classes as a bitset), then
 *     loss = alpha / (mh mw) * sum over b, c, pixels of max(x, 0) - x t + log1p(exp(-|x|))        (BCE with logits)
 *     d_segm = alpha / (mh mw) * (sigmoid(x) - t)
 * An image without objects is valid (target 0), and so is G = 0.  A label outside 0 .. K-1 sets no bit and makes loss NaN.  No
 * atomics: the same inputs give the same bits.  The offsets are given on the device and on the host as in ymi_match_desc.
 * YMI_EARG: B outside 1..65535, K outside 1..128, mh / mw < 1, G < 0, offsets that do not start at 0, end at G or decrease;
 * YMI_ESHAPE: B*K*mh*mw >= 2^31 (for B = K = 1: mh*mw > 2^31 - 256), segm / d_segm / ws not 16-byte aligned; YMI_ENULL: segm, gt_off, gt_off_host, loss or ws NULL,
 * or (G > 0) gt or label NULL.  No error path launches anything. */
typedef struct ymi_segm_loss_desc {
  const float *segm;            /* [B,K,mh,mw] NCHW logits, the layout semantic_seg_conv produces */
  const uint8_t *gt;            /* [G,mh,mw] 0 / non-zero: the downsampled, binarised GT masks of the batch, image by image */
  const int32_t *label;         /* [G] class of each mask, 0..K-1 */
  const int32_t *gt_off;        /* DEVICE [B+1]: the masks of image b are [gt_off[b], gt_off[b+1]) */
  const int32_t *gt_off_host;   /* HOST   [B+1]: the same values */
  float *loss;                  /* [1] */
  float *d_segm;                /* [B,K,mh,mw]; may be NULL */
  void *ws;                     /* ymi_workspace_bytes(YMI_WS_SEGM_LOSS, desc) bytes, 16-byte aligned */
  int32_t B, K, mh, mw, G;
  float alpha;                  /* cfg.semantic_segmentation_alpha */
} ymi_segm_loss_desc;
int ymi_segm_loss_f32(const ymi_segm_loss_desc *d, void *stream);

/* -- the mask-IoU term 'I' of YOLACT++ (layers/modules/multibox_loss.py:629-672, 684-694; csrc/maskiou_loss.hip; additive at ABI 9) --
 * fp32 throughout, no floating-point atomics: the same inputs give the same bits.  No error path launches anything.
 *
 * ymi_maskiou_input_f32: the instances as ymi_mask_loss_f32 takes them -> the net's input and its targets, one launch:
 *     x0[j,r,c] = inside_j(r,c) ? sigmoid(sum_k proto[b,r,c,k] coef[j,k]) : 0      (the crop window of ymi_mask_loss_f32, padding 1)
 *     iou_t[j]  = inter / ((a1 + a2) - inter):  a1 = window pixels with logit > 0, a2 = set pixels of the whole GT row, inter = both
 * The reference binarises sigmoid > 0.5 in fp32; logit > 0 is the same decision except for logits in (0, ~6e-8], whose fp32
 * sigmoid rounds to 0.5.  A union of 0 gives the reference's NaN.
 * ymi_maskiou_input_bwd_f32: g = inside ? d_x0 p (1 - p) : 0;  d_proto[b,pix,k] = sum_j g coef[j,k] (every element written),
 *     d_coef[j,k] = sum_pix g proto[b,pix,k]; either may be NULL, not both.  Two launches (one without d_coef).
 * YMI_ESHAPE: K != 32, mh*mw >= 2^24, N >= 2^24, proto / d_proto / ws not 16-byte aligned, ws_bytes too small; YMI_EARG: B outside
 * 1..65535, mh / mw / N / G < 1, img_off_host not starting at 0, ending at N or decreasing; YMI_ENULL: a pointer the call reads or
 * writes is NULL. */
typedef struct ymi_maskiou_input_desc {
  const float *proto;           /* [B,mh,mw,K] */
  const float *coef;            /* [N,K] */
  const float *box;             /* [N,4] relative point form */
  const uint8_t *gt;            /* [G,mh,mw] 0 / non-zero (forward only) */
  const int32_t *gt_idx;        /* [N] row of gt, clamped to 0..G-1 (forward only) */
  const int32_t *img_off;       /* DEVICE [B+1]: the instances of image b are [img_off[b], img_off[b+1]) */
  const int32_t *img_off_host;  /* HOST   [B+1]: the same values */
  float *x0;                    /* [N,mh,mw] (forward) */
  float *iou_t;                 /* [N] (forward) */
  const float *d_x0;            /* [N,mh,mw] (backward) */
  float *d_proto;               /* [B,mh,mw,K] (backward; may be NULL) */
  float *d_coef;                /* [N,K] (backward; may be NULL) */
  void *ws;                     /* backward with d_coef: ymi_workspace_bytes(YMI_WS_MASKIOU_INPUT, desc) bytes, 16-byte aligned */
  int64_t ws_bytes;
  int32_t B, mh, mw, K, N, G;
} ymi_maskiou_input_desc;
int ymi_maskiou_input_f32(const ymi_maskiou_input_desc *d, void *stream);
int ymi_maskiou_input_bwd_f32(const ymi_maskiou_input_desc *d, void *stream);

/* The backward of y = relu?(conv(x, w) + b) as ymi_conv2d_direct_nhwc_f32 computes it, for any kernel size, stride and padding it
 * accepts.  With relu = 1, dy is first masked by y > 0 (y = the layer's post-ReLU output).
 *     dx[n,iy,ix,ci] = sum over the output pixels that read (iy, ix), taps in (ky, kx) order, of sum_co dy w[(ky kw + kx) Cin + ci, co];
 *                      a pixel no window reaches gets an exact zero.  One launch.
 *     dw[k,co] = sum_pos im2col(x)[pos,k] dy[pos,co], db[co] = sum_pos dy[pos,co], pos = (n, oy, ox) in order: the positions are cut
 *                      into chunks whose partial sums go to ws (launch one: the tile of [K + 1, Cout] a block owns and the number
 *                      of chunks follow the shape) and are added in chunk order (launch two).
 * dx, or dw and db together, may be NULL.  w and dw are [kh*kw*Cin, ceil4(Cout)], the forward's layout (dw's padding columns are
 * written as zeros).  YMI_EARG: a size < 1, pad < 0, relu not 0 / 1; YMI_ESHAPE: Ho / Wo not the convolution's, w / y / dy / ws not
 * 16-byte aligned, ws_bytes too small, more than 65535 tiles of [K + 1, Cout] (tiles of 64 x 64 for wide layers); YMI_ENULL: dy NULL, y NULL with relu, nothing to compute, w NULL with dx, x or ws NULL with dw / db. */
typedef struct ymi_conv_bwd_desc {
  const float *x;               /* [B,H,W,Cin] */
  const float *w;               /* [kh*kw*Cin, ceil4(Cout)], k = (ky*kw + kx)*Cin + ci */
  const float *y;               /* [B,Ho,Wo,Cout] */
  const float *dy;              /* [B,Ho,Wo,Cout] */
  float *dx;                    /* [B,H,W,Cin] */
  float *dw;                    /* [kh*kw*Cin, ceil4(Cout)] */
  float *db;                    /* [Cout] */
  void *ws;                     /* ymi_workspace_bytes(YMI_WS_CONV_BWD, desc) bytes, 16-byte aligned */
  int64_t ws_bytes;
  int32_t B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, relu;
} ymi_conv_bwd_desc;
int ymi_conv2d_bwd_nhwc_f32(const ymi_conv_bwd_desc *d, void *stream);

/* The backward of ymi_global_maxpool_nhwc_f32: dy[n,q,c] = d_pool[n,c] at the FIRST q (row-major) where y[n,q,c] is the maximum, 0
 * elsewhere: the tie rule of torch's CPU max_pool2d. */
int ymi_global_maxpool_bwd_nhwc_f32(const float *y, const float *d_pool, float *dy, int B, int HW, int C, void *stream);

/* The head of 'I': p_n = pool[n,label[n]], loss = alpha sum_n smooth_l1(p_n - iou_t[n]) (beta 1, summed in ymi's fixed tree),
 * d_pool[n,c] = c == label[n] ? alpha smooth_l1'(p_n - iou_t[n]) : 0.  Two launches.  YMI_EARG: N / C < 1; YMI_ESHAPE: ws_bytes too
 * small; YMI_ENULL: pool, iou_t, label, loss or ws NULL. */
typedef struct ymi_maskiou_head_desc {
  const float *pool;            /* [N,C] */
  const float *iou_t;           /* [N] */
  const int32_t *label;         /* [N], clamped to 0..C-1 */
  float *loss;                  /* [1] */
  float *d_pool;                /* [N,C]; may be NULL */
  void *ws;                     /* ymi_workspace_bytes(YMI_WS_MASKIOU_HEAD, desc) bytes */
  int64_t ws_bytes;
  int32_t N, C;
  float alpha;                  /* cfg.maskiou_alpha */
  int32_t _pad0;
} ymi_maskiou_head_desc;
int ymi_maskiou_head_f32(const ymi_maskiou_head_desc *d, void *stream);

/* -- the backward of the train-mode heads and protonet (csrc/conv_train.hip; additive, the ABI number stays) -----------------------
 * and of the train-mode FPN (yolact.py:311-360: ymi_conv_wgrad_desc.stride, ymi_bilinear_size_bwd_nhwc_f32).
 * Stride-1 convolutions (3x3 / pad 1, 1x1 / pad 0), ReLU, tanh and the x2 bilinear upsample (yolact.py:133-212, 580-647).  No
 * floating-point atomics anywhere: the same inputs give the same bits.  The DATA gradient of such a convolution is
 * ymi_conv2d_nhwc_f32 on g with the filters flipped in both taps and transposed in (Cin, Cout); it has no entry of its own.
 *
 * ymi_act_bwd_f32: g[pos,c] = dy[pos,c] * act'(y[pos,c]) for c < C from the layer's OUTPUT y (YMI_ACT_RELU: y > 0 ? 1 : 0,
 * YMI_ACT_TANH: 1 - y^2, YMI_ACT_NONE: 1, y may be NULL), g[pos,c] = 0 for C <= c < cpad.  ldy / lddy / ldg: the channel strides.
 * YMI_EARG: another activation, npos / C < 1; YMI_ESHAPE: cpad < C, ldg < cpad, lddy < C, ldy < C; YMI_ENULL: dy, g, or y with an
 * activation. */
int ymi_act_bwd_f32(const float *y, const float *dy, float *g, long npos, int C, int cpad, int ldy, int lddy, int ldg, int act,
                    void *stream);

/* dw[k,co] = sum_pos im2col(x)[pos,k] g[pos,co] (k = (ky*kw + kx)*Cin + ci), db[co] = sum_pos g[pos,co], pos = (n, oy, ox), on the
 * exact-fp32 matrix instruction with the positions as its k index.  The positions are cut into chunks whose partial sums go to ws
 * (launch one) and are added in chunk order (launch two).  dw or db may be NULL.  YMI_EARG: a size < 1, a geometry other than
 * 3x3 / pad 1 and 1x1 / pad 0; YMI_ESHAPE: Cin % 32, ldg < Cout, x or g of 2^29 elements or more (2 GiB, the conv engine's limit), ws not 16-byte aligned, ws_bytes
 * too small; YMI_ENULL: g or ws NULL, nothing to compute, x NULL with dw.  No error path launches anything.
 * stride = 2 (the FPN's downsample layers, the backbone's stage entries): g is [B,Ho,Wo,ldg] with Ho = (H + 2 pad - kh) / 2 + 1, the
 * positions (n, oy, ox) are those of g, and tap (ky, kx) reads x at (2 oy + ky - pad, 2 ox + kx - pad), 0 outside the map (on an odd H
 * the bottom row of taps of the last output row falls outside).  The chunks, hence the workspace, follow the positions of g; the
 * chunk-ordered second pass, the db rule and the 2^29 limits (x, and g over its own positions) are those of stride 1.  YMI_EARG: a
 * stride other than 0, 1, 2. */
typedef struct ymi_conv_wgrad_desc {
  const float *x;               /* [B,H,W,Cin] */
  const float *g;               /* [B,Ho,Wo,ldg] (Ho = H, Wo = W at stride 1), channels [0, Cout) are read */
  float *dw;                    /* [kh*kw*Cin, Cout] */
  float *db;                    /* [Cout] */
  void *ws;                     /* ymi_workspace_bytes(YMI_WS_CONV_WGRAD, desc) bytes, 16-byte aligned */
  int64_t ws_bytes;
  int32_t B, H, W, Cin, Cout, ldg, kh, kw, pad;
  int32_t stride;               /* 0 or 1: stride 1 (callers from before the field had a name leave it 0); 2: stride 2 */
} ymi_conv_wgrad_desc;
int ymi_conv_wgrad_nhwc_f32(const ymi_conv_wgrad_desc *d, void *stream);

/* The same weight gradient on the fp16 matrix pipe, opt-in (csrc/conv_wgrad_h2.hip; additive, the ABI number stays).  The descriptor,
 * dw, db, ldg, stride, the accepted shapes and every error code are those of ymi_conv_wgrad_nhwc_f32; ws is
 * ymi_workspace_bytes(YMI_WS_CONV_WGRAD_H2, desc) bytes.  No error path launches anything.  The bits differ from the fp32 entry's
 * and are equal on every run: no floating-point atomics, the order of additions is a function of the shape only.
 *   Operands  "fp16x2" (csrc/gemm_h2.h): per element t = v * s, h = fp16(t), l = fp16(t - h), both by round to nearest; s is one
 *             power of two per tensor, the one that puts the tensor's magnitude bound into [2^13, 2^14) (a bound of 0, Inf or NaN:
 *             s = 1).  The bounds, max |x| over all of x and max |g| over the channels [0, Cout) only (channels [Cout, ldg) may hold
 *             anything, NaN included: they are never part of a sum), are computed on the device inside the call, into ws; there is
 *             no host read and no synchronisation.
 *   dw        A block owns one (tap, 32 input channels), one chunk of positions and 128 (Cout <= 128) or 256 output channels.  The
 *             positions are cut into chunks by the fp32 entry's rule (csrc/grad_common.h: about 1024 blocks in all when
 *             kh kw (Cin / 32) G blocks work on every chunk) with G = ceil(Cout / 128) for Cout <= 128 and ceil(Cout / 256)
 *             above: the fp32 entry's very chunks up to Cout = 256, more and shorter ones above it.  Within a chunk the positions
 *             go in K-steps of 16, ascending; per K-step and element the fp32 accumulator takes, in this order,
 *             sum16(xh gh), sum16(xh gl), sum16(xl gh) (v_mfma_f32_32x32x16_f16: exact products, fp32 accumulation; xl gl is
 *             dropped, <= 2^-22 |x g|).  The chunk partials are added in chunk order from +0.0, and the sum is multiplied by
 *             2^(e >> 1), then by 2^(e - (e >> 1)), 2^e = 1 / (s_x s_g): the product of the scales is never formed, so operands of
 *             2^-60 or 2^50 keep an fp32-class result.  A bound of 0 gives dw = +0.0 in every element; an Inf or NaN in column co of
 *             g makes dw[:,co] non-finite.
 *   db        Plain fp32, no split, from the same call: per chunk, the positions 16 q + 0 .. 7 (all q ascending) and
 *             16 q + 8 .. 15 as two running sums, the first plus the second; the chunk partials in chunk order from +0.0. */
int ymi_conv_wgrad_nhwc_h2(const ymi_conv_wgrad_desc *d, void *stream);

/* The filters of a training step as the fp16x2 tiles of ymi_conv2d_nhwc_f32 read them (ymi_conv_desc.w_h2 / scale_h2 / winv_h2), packed
 * ON THE DEVICE from the parameters' current storage (csrc/conv_pack_h2.hip; additive, the ABI number stays).  w[i], i < n <= 3, are
 * fp32 [cout[i], Cin, k, k] in torch layout, contiguous, any 4-byte alignment, read in place; their output channels are concatenated,
 * Rows below is the row count, RowsPad = ceil128(Rows).
 *   mode 0    the forward's filters: row = output channel, Rows = sum cout, Kp = k k Cin, column (ky k + kx) Cin + c.
 *   mode 1    the data gradient's: row = input channel, Rows = Cin, Kp = k k ld, column (ky' k + kx') ld + co holds
 *             w[co, row, k - 1 - ky', k - 1 - kx'] (both taps flipped), co over the concatenated outputs, columns co in [sum cout, ld)
 *             zero (ld: the channel stride of the backward's g).
 *   planes    int16 [2][RowsPad][Kp]: plane 0 = fp16(w s_row), plane 1 = fp16(w s_row - plane 0), both by round to nearest even (the
 *             difference is exact in fp32; csrc/gemm_h2.h split8h does the same to the activations).
 *   winv      fp32 [RowsPad] = 1 / s_row.  s_row is the scale that ymi_h2_scale of csrc/common.h gives the row's max |w|: the power of two that puts it
 *             into [2^13, 2^14), clamped to [2^-125, 2^125]; a row maximum of 0, Inf or NaN (a NaN anywhere in the row counts) gives
 *             s_row = 1, the helper's rule, so an Inf or NaN stays one in plane 0.  For every row whose maximum is a normal number in
 *             [2^-100, 2^100] the result equals engine.split2_planes_f16 of the torch packing bit for bit.
 *   w32       optional (NULL: not written) fp32 [RowsPad][Kp]: the same packing unsplit, ymi_conv_desc.w of the fp32 tiles.  The fp16x2
 *             tiles never read ymi_conv_desc.w; the entry's validation only wants it non-NULL and 16-byte aligned.
 * Rows [Rows, RowsPad) are written too: planes (and w32) zero, winv 1.  Every element of every output is written, once.  One launch,
 * no atomics, no workspace: a block owns whole rows (mode 0: one; mode 1: 8 input channels), finds their maxima in a first pass
 * over the source and splits in a second; both passes read the source in contiguous runs and transpose through LDS.
 * YMI_ENULL: d, planes, winv or one of w[0 .. n) NULL; YMI_EARG: n outside 1 .. 3, k not 1 or 3, mode not 0 or 1, Cin or a cout < 1;
 * YMI_ESHAPE: Cin % 32, in mode 1 ld % 32 or ld < sum cout, planes / winv / w32 not 16-byte aligned, RowsPad Kp >= 2^29.  Validation
 * runs on the host before any HIP call; no error path launches anything. */
typedef struct ymi_conv_pack_desc {
  const float *w[3];            /* [cout[i], Cin, k, k] */
  void *planes;                 /* int16 [2][RowsPad][Kp] */
  float *winv;                  /* [RowsPad] */
  float *w32;                   /* NULL, or [RowsPad][Kp] */
  int32_t cout[3];
  int32_t n, Cin, k;
  int32_t mode;                 /* 0: forward, 1: data gradient */
  int32_t ld;                   /* mode 1: the padded output-channel count; mode 0: unused */
} ymi_conv_pack_desc;
int ymi_conv_pack_h2_f32(const ymi_conv_pack_desc *d, void *stream);

/* The backward of ymi_bilinear_nhwc_f32 (align_corners=False, optional ReLU: dy is masked by y > 0, y = its output) for Ho = 2 Hi,
 * Wo = 2 Wi, odd sizes included, as a gather: dx[b,iy,ix,c] sums the output pixels that read (iy, ix), rows then columns in order,
 * with the coordinates of the forward.  YMI_ESHAPE: another ratio, C % 4, a pointer not 16-byte aligned; YMI_EARG: a size < 1, relu
 * not 0 / 1; YMI_ENULL: dy, dx, or y with relu. */
int ymi_bilinear_bwd_nhwc_f32(const float *dy, const float *y, float *dx, int B, int Hi, int Wi, int C, int Ho, int Wo, int relu,
                              void *stream);

/* The backward of y = F.interpolate(x, size=(Ho, Wo), mode='bilinear', align_corners=False) (ymi_bilinear_nhwc_f32 with scale 0, the
 * FPN's top-down step, yolact.py:332) for ANY Ho >= Hi and Wo >= Wi, Ho = Hi (the identity: dx = dy bit for bit) and Hi = 1 included;
 * the scale is (float)Hi / (float)Ho.  A gather: one thread per (input pixel, 4 channels) inverts the coordinate map into a
 * conservative range of candidate output rows and columns, asks the forward's own fp32 coordinates (upsample_math.h up_coord) which
 * of them read its pixel, and adds (1 - l1) dy where i0 is its index and l1 dy where i1 is (both at the clamped last row).
 * SUMMATION ORDER (part of the contract): output rows ascending, within a row output columns ascending, each term (wy * wx) * dy.
 * Every element of dx is written; no atomics.  YMI_ENULL: dy or dx NULL; YMI_EARG: a size < 1; YMI_ESHAPE: Ho < Hi, Wo < Wi, C % 4,
 * a pointer not 16-byte aligned, 2^40 elements of dy or more.  No error path launches anything. */
int ymi_bilinear_size_bwd_nhwc_f32(const float *dy, float *dx, int B, int Hi, int Wi, int C, int Ho, int Wo, void *stream);

/* -- the backward of the train-mode backbone (csrc/conv_dgrad.hip, csrc/bn_train.hip; additive, the ABI number stays) -------------------
 * ymi_conv_dgrad_s2_nhwc_f32: the data gradient of a STRIDE-2 convolution, 3x3 / pad 1 or 1x1 / pad 0 (each ResNet stage's first conv2
 * and the projection shortcuts): dx[n,y,x,ci] = sum over the taps (ky, kx) that exist for the pixel of sum_co g[n,oy,ox,co] w[co,ci,ky,kx],
 * oy = (y + pad - ky) / 2 where exact and inside [0, Ho), Ho = (H + 2 pad - kh) / 2 + 1 (odd and even H, W).  Only existing taps are
 * computed: the four parity phases (y & 1, x & 1) of a 3x3 have 1, 2, 2 and 4 taps, 9 tap-products per 2 x 2 pixels (the zero-insert
 * route over ymi_conv2d_nhwc_f32 spends 36); a tap whose oy or ox lies outside g (the last odd row / column of an even extent) is
 * masked.  At 1x1 the even / even pixels get one product and every other pixel an exact +0.0.  On v_mfma_f32_32x32x2_f32 (fp32 in,
 * fp32 accumulate) with Cout as its k index.  w is PACKED by the caller from the current values: [kh][kw][Cout / 4][Cin][4] with
 * element (ky, kx, co / 4, ci, co % 4) = weight[co, ci, ky, kx].  g's channels [0, Cout) are read; [Cout, ldg) may hold anything.
 * SUMMATION ORDER (part of the contract, a function of the shape only): an element starts from +0.0 and adds its taps with ky
 * ascending, within ky kx ascending; within a tap q = 0 .. Cout / 8 - 1 ascending, within q e = 0 .. 3, and step (q, e) adds the two
 * products of co = 8 q + e and co = 8 q + 4 + e in one instruction.  Every element of dx is written, once; no atomics; the same inputs
 * give the same bits.  YMI_EARG: a size < 1, another geometry, stride != 2; YMI_ESHAPE: Cin % 32, Cout % 32, ldg < Cout, ldg % 4, 2^29
 * elements or more in g, dx or w, a pointer not 16-byte aligned; YMI_ENULL: a NULL pointer.  No error path launches anything. */
typedef struct ymi_conv_dgrad_desc {
  const float *g;               /* [B,Ho,Wo,ldg] */
  const float *w;               /* [kh][kw][Cout/4][Cin][4] */
  float *dx;                    /* [B,H,W,Cin] */
  int32_t B, H, W, Cin, Cout, ldg, kh, kw, pad;
  int32_t stride;               /* 2 */
} ymi_conv_dgrad_desc;
int ymi_conv_dgrad_s2_nhwc_f32(const ymi_conv_dgrad_desc *d, void *stream);

/* BatchNorm2d on its own, NHWC fp32 viewed as [npos, C], C % 4 == 0; one descriptor for both directions.
 * ymi_bn_fwd_nhwc_f32, training = 1: mean_c and the biased var_c over npos, invstd = 1 / sqrt(var + eps),
 * y = gamma (x - mean) invstd + beta (+ res) (then ReLU when relu = 1); mean and invstd are written for the backward; running_mean /
 * running_var (may be NULL) become (1 - momentum) r + momentum stat, with the unbiased variance var npos / (npos - 1).  The variance is
 * the mean of squared deviations about the mean (two passes over x; never E[x^2] - E[x]^2), and the sums run over x - x[0, c].
 * training = 0 (frozen): mean = running_mean, invstd = 1 / sqrt(running_var + eps), the same map; mean / invstd are written, nothing
 * is updated.
 * ymi_bn_bwd_nhwc_f32: gh = dy [y > 0] with relu (y = the forward's output), else dy; d_res = gh; dbeta = sum gh; dgamma = sum gh xh,
 * xh = (x - mean) invstd; dx = gamma invstd (gh - dbeta / npos - xh dgamma / npos) (training: the sums are always formed) or
 * gamma invstd gh (frozen).  dx, d_res, dgamma, dbeta may each be NULL.
 * COLUMN SUMS (part of the contract): chunks of per = max(32, ceil(npos / 1024)) positions; a chunk's positions are added in ascending
 * order from +0.0; of the chunk partials (in ws) of a channel, lane l of one wave adds the chunks l, l + 64, .. in ascending order from
 * +0.0 and the 64 lane sums are added by a butterfly over the lane distances 32, 16, 8, 4, 2, 1.  No atomics; the same inputs give the same bits.
 * YMI_EARG: npos / C < 1, training or relu not 0 / 1, eps < 0, training = 1 with npos < 2 (PyTorch refuses it too); YMI_ESHAPE: C % 4,
 * 2^40 elements or more, a pointer not 16-byte aligned, ws_bytes too small; YMI_ENULL: a pointer the call needs (forward: x, gamma,
 * beta, y, mean, invstd, ws, and the running statistics when frozen; backward: dy, ws, y with relu, x / mean / invstd for the sums or
 * dx, gamma for dx, at least one result).  No error path launches anything. */
typedef struct ymi_bn_desc {
  const float *x;               /* [npos,C] */
  const float *res;             /* [npos,C] or NULL (forward) */
  const float *gamma, *beta;    /* [C] */
  float *running_mean, *running_var;   /* [C]; updated in place when training */
  float *y;                     /* [npos,C]: the forward's result; read by the backward when relu */
  float *mean, *invstd;         /* [C]: written by the forward, read by the backward */
  const float *dy;              /* [npos,C] (backward) */
  float *dx, *d_res;            /* [npos,C] or NULL */
  float *dgamma, *dbeta;        /* [C] or NULL */
  void *ws;                     /* ymi_workspace_bytes(YMI_WS_BN, desc) bytes, 16-byte aligned */
  int64_t ws_bytes;
  int64_t npos;
  int32_t C, training, relu;
  float eps, momentum;
  int32_t _pad0;
} ymi_bn_desc;
int ymi_bn_fwd_nhwc_f32(const ymi_bn_desc *d, void *stream);
int ymi_bn_bwd_nhwc_f32(const ymi_bn_desc *d, void *stream);

/* -- the backward of the train-mode ResNet stem (csrc/stem_train.hip; additive, the ABI number stays) -----------------------------------
 * backbone.py:129-132: conv1 7x7 / stride 2 / pad 3 on 3 channels, bn1, ReLU, MaxPool2d(3, 2, 1).  The forward convolution is
 * ymi_conv2d_nhwc_f32 with Cin = 4 (the fourth input channel of the filter zero), bn1 + ReLU are ymi_bn_fwd_nhwc_f32 / ymi_bn_bwd_nhwc_f32.
 * No atomics; every element of every output is written exactly once; the same inputs give the same bits.
 *
 * ymi_stem_wgrad_nhwc_f32: dw[k,co] = sum_pos x[n, 2 oy + ky - 3, 2 ox + kx - 3, ci] g[pos,co], k = (ky*7 + kx)*3 + ci (147 rows),
 * pos = [n, oy, ox] over the positions of g, Ho = [H - 1] / 2 + 1 and Wo likewise, reads outside the image are 0.  x is the NHWC-4 image
 * the forward's Cin-4 loader reads; its channel 3 is padding and reaches no row of dw WHATEVER IT HOLDS (a select, never a product).
 * On v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate) with the positions as its k index.  No data gradient: nothing upstream of the
 * image needs one.
 * SUMMATION ORDER (part of the contract, a function of the shape only): the positions n-major, then oy, then ox, are cut into chunks of
 * per = 32 ceil(ceil(P / 32) / min(ceil(P / 32), ceil(512 / ceil(Cout / 64)))) positions, P = B Ho Wo.  A chunk's partial sum starts from
 * +0.0 and takes its positions in ascending order two at a time: one instruction adds the two products of positions p and p + 1
 * (p - chunk start even; a position outside the image or past the chunk contributes an exact 0 product).  The partials go to ws and a
 * second launch adds them in chunk order from +0.0.
 * YMI_ENULL: the descriptor, x, g, dw or ws NULL; YMI_EARG: B, H, W or Cout < 1; YMI_ESHAPE: Cout % 32, ldg < Cout, ldg % 4, x or g of
 * 2^29 elements or more, ws not 16-byte aligned, ws_bytes too small.  No error path launches anything. */
typedef struct ymi_stem_wgrad_desc {
  const float *x;               /* [B,H,W,4] */
  const float *g;               /* [B,Ho,Wo,ldg], channels [0, Cout) are read */
  float *dw;                    /* [147, Cout] */
  void *ws;                     /* ymi_workspace_bytes(YMI_WS_STEM_WGRAD, desc) bytes, 16-byte aligned */
  int64_t ws_bytes;
  int32_t B, H, W, Cout, ldg, _pad0;
} ymi_stem_wgrad_desc;
int ymi_stem_wgrad_nhwc_f32(const ymi_stem_wgrad_desc *d, void *stream);

/* MaxPool2d(3, 2, 1) on x [B,H,W,C] NHWC fp32 and its backward, C % 4 == 0, any H, W >= 1: y, dy are [B,Hp,Wp,C], Hp = [H - 1] / 2 + 1.
 * Padding never wins (a window always holds a real pixel).  TIE RULE (part of the contract): of equal maxima the FIRST in row-major
 * window order (ky, then kx) is the maximum's place and takes the gradient, as PyTorch's max_pool2d does; NaN inputs are outside the
 * contract.
 * ymi_maxpool_bwd_nhwc_f32 is a gather that keeps no argmax plane: it RECOMPUTES the argmax of each window from x (the forward's input,
 * unchanged since).  An input pixel lies in 1, 2, 2 or 4 windows by its row and column parity; it starts from +0.0 and adds dy of
 * those windows whose argmax it is, output rows ascending, within a row output columns ascending.  No ReLU mask is applied here
 * (ymi_bn_bwd_nhwc_f32 with relu = 1 applies it).
 * YMI_ENULL: a NULL pointer; YMI_EARG: B, H, W or C < 1; YMI_ESHAPE: C % 4, 2^40 elements of x or more, a pointer not 16-byte aligned.
 * No error path launches anything. */
int ymi_maxpool_fwd_nhwc_f32(const float *x, float *y, int B, int H, int W, int C, void *stream);
int ymi_maxpool_bwd_nhwc_f32(const float *x, const float *dy, float *dx, int B, int H, int W, int C, void *stream);

/* -- ResNet stem in one launch (backbone.py:126-133 + the layout change of yolact.py:564) ---------------------------------
 * x [B,3,H,W] NCHW fp32 (the normalised image) -> conv 7x7 / 2 / pad 3 (3 -> 64) + folded BN + ReLU -> max-pool 3x3 / 2 / pad 1
 * -> y [B,Hp,Wp,64] NHWC fp32, Hp = ((H - 1) / 2 + 1 - 1) / 2 + 1.  The 64-channel stem output stays in LDS (csrc/stem.hip).
 * fp16x2 arithmetic: filters as the two fp16 planes of engine.Packed(cin_pad = 4).h2() (k = (7 ky + kx) * 4 + c, Kpad 224);
 * the input is scaled per tile from the tile's own maximum, so no magnitude bound of x is needed; y_amax as in ymi_conv_desc. */
typedef struct ymi_stem_desc {
  const float *x;        /* [B,3,H,W] */
  float *y;              /* [B,Hp,Wp,64] */
  int32_t B, H, W, cout_pad;
  const void *w_h2;      /* fp16 planes [2][cout_pad][kpad] */
  const float *scale_h2, *bias;
  float *y_amax;         /* magnitude-bound slot of y (may be NULL) */
  int32_t kpad, _pad0;   /* 224 */
} ymi_stem_desc;
int ymi_stem_pool_f32(const ymi_stem_desc *d, void *stream);

/* -- two chained 1x1 convolutions of a ResNet stage in one launch (csrc/chain.hip: 64 planes; csrc/chain2.hip, ABI 8: 128 / 256) --
 *     y = act_a(scale_a * (W_a x) + bias_a + res)      conv3 + bn3 + shortcut + ReLU of Bottleneck b   (backbone.py:49-55)
 *     z = act_b(scale_b * (W_b y) + bias_b)            conv1 + bn1 + ReLU of Bottleneck b + 1          (backbone.py:41-43)
 * x [M,ldx] (k_a = 64 channels), res [M,res_ld] or NULL, y [M,ldy] (n_a = 256), z [M,ldz] (n_b = 64) or NULL (then only y is
 * computed): NHWC rows, M = B*H*W.  Filters as the fp16x2 planes of the two layers (ymi_conv_desc.w_h2 / scale_h2: planes
 * [2][cout_pad][K]); x_amax / y_amax / z_amax as in ymi_conv_desc (x_amax required).  y is written once and never read back:
 * the second GEMM takes it from LDS.
 * ALIASING: y and z must not overlap each other, res or (for y) x.  z MAY be x exactly in place — z == x and ldz == ldx — and in no
 * other overlapping form: a block reads x rows [32 t, 32 t + 32) before it writes the same rows of z and no other block touches
 * them; any other overlap lets one block's z rows land on x rows another block has not read yet (engine.Plan checks this before
 * it fuses two launches into this one; the library does not). */
typedef struct ymi_chain_desc {
  const float *x, *res;
  float *y, *z;
  const void *w_a_h2, *w_b_h2;
  const float *scale_a_h2, *bias_a, *scale_b_h2, *bias_b;   /* biases may be NULL */
  const float *x_amax;
  float *y_amax, *z_amax;                                    /* may be NULL */
  int64_t M;
  int32_t ldx, res_ld, ldy, ldz;
  int32_t k_a, n_a, n_b;                                     /* (P, 4P, P) with P = 64 (csrc/chain.hip), 128 or 256 (csrc/chain2.hip) */
  int32_t cout_pad_a, cout_pad_b;                            /* rows per filter plane (engine.Packed.CoutPad) */
  int32_t act_a, act_b, _pad0;                               /* YMI_ACT_NONE / RELU / LEAKY01 */
  /* ABI 8, P = 128 / 256 only (ignored at P = 64): the y slices of a block feed ONE accumulation of z and therefore share one
   * power-of-two scale, derived when the kernel starts from a rigorous bound of y:
   *     |y| <= amax(x) * gain_a + bias_max_a + amax(res)
   * gain_a = max_n(|folded BN scale_n| * sum_k |w_a[n, k]|) (> 0), bias_max_a = max_n |bias_a[n]| (>= 0), both from the fp32
   * filters (engine.Packed.l1_gain()); res_amax = the magnitude-bound slot of the residual tensor (required when res != NULL). */
  const float *res_amax;
  float gain_a, bias_max_a;
  /* additive within ABI 9, P = 64 only: the ENTRY form (csrc/chain.hip, chain_h2_k<64, true>).  All zero = the launch above, bit
   * for bit.  x0 != NULL: the residual is not read but COMPUTED in the launch as the block's projection shortcut (backbone.py:52-53),
   *     res = scale_d * (W_d x0) + bias_d              1x1, stride 1, 64 -> 256, no activation
   * from the block input x0 [M,ldx0] (64 channels; ldx0 >= 64) with x0's OWN magnitude slot x0_amax (required; independent of
   * x_amax); w_d_h2 / scale_d_h2 / bias_d / cout_pad_d as the other two layers'.  y = act_a(scale_a * (W_a x) + bias_a + res) in
   * that expression order: against the shortcut through ymi_conv2d_nhwc_f32 followed by this launch with `res` only the summation
   * order inside W_d x0 differs.  z may be NULL.
   * Requires res == NULL and (k_a, n_a) = (64, 256), else YMI_EARG (ymi_stage_exit_chain_f32 and the P = 128 / 256 path refuse a
   * descriptor with x0 set: YMI_EARG); w_d_h2, scale_d_h2, x0_amax, else YMI_ENULL; ldx0 >= 64 and % 4 == 0, x0 / w_d_h2 16-byte
   * aligned, M * ldx0 < 2^29, cout_pad_d >= 256, else YMI_ESHAPE.
   * ALIASING, beside the rules above: y must not overlap x0.  z MAY be x0 exactly in place — z == x0 and ldz == ldx0 — for the
   * reason given for x (a block reads rows [32 t, 32 t + 32) of x0 before it writes those rows of z), and in no other overlapping
   * form; the arena can hand conv1's output the buffer of the block input, so engine.Plan checks this before it fuses. */
  const float *x0, *x0_amax;
  const void *w_d_h2;
  const float *scale_d_h2, *bias_d;                          /* bias_d may be NULL */
  int32_t ldx0, cout_pad_d;
} ymi_chain_desc;
int ymi_pointwise_chain_f32(const ymi_chain_desc *d, void *stream);

/* -- the EXIT of the first ResNet stage in one launch (csrc/chain.hip, chain_h2_k<128>; additive within ABI 9) ---------------------
 *     y = act_a(scale_a * (W_a x) + bias_a + res)      conv3 + bn3 + shortcut + ReLU of the stage's last Bottleneck (64 -> 256)
 *     z = act_b(scale_b * (W_b y) + bias_b)            conv1 + bn1 + ReLU of the next stage's first Bottleneck    (256 -> 128)
 * `chain` is read as in ymi_pointwise_chain_f32 with (k_a, n_a, n_b) = (64, 256, 128) and z REQUIRED (gain_a / bias_max_a /
 * res_amax are ignored).  chain.M == B * H * W.  y_stride = 1: y is stored for every pixel; y_stride = 2: a row of y is stored
 * only where h % 2 == 0 && w % 2 == 0 — what a 1x1 stride-2 reader (the next stage's projection shortcut) touches — and the other
 * rows of y are NOT WRITTEN AT ALL.  Either way y_amax bounds y over EVERY pixel and z (with z_amax) is written for every pixel.
 * ALIASING: z must not overlap x, res or y; there is no in-place form (z is wider than x).  y must not overlap x or res.
 * Codes: NULL descriptor / pointer -> YMI_ENULL; (k_a, n_a, n_b) != (64, 256, 128), y_stride not 1 or 2, M != B*H*W, an unknown
 * activation -> YMI_EARG; row pitches / 16-byte alignment / 32-bit offsets / filter-plane rows -> YMI_ESHAPE.
 * LIMIT: M * max(H, W) < 2^32, otherwise YMI_ESHAPE (the kernel finds a row's (h, w) by a 32-bit reciprocal multiplication that is
 * exact only below that; 16 x 138 x 138 x 138 = 4.2e7). */
typedef struct ymi_stage_exit_desc {
  ymi_chain_desc chain;
  int32_t B, H, W, y_stride;
} ymi_stage_exit_desc;
int ymi_stage_exit_chain_f32(const ymi_stage_exit_desc *d, void *stream);

/* -- native plan executor (ABI 7; csrc/plan_exec.cpp) ----------------------------------------------------------------------------
 * The engine's execution plan is a flat list of the calls above on two HIP streams (A = the caller's stream, B = a side stream
 * for the small P4..P7 / Detect / projection-shortcut launches) with record / wait markers between them.  ymi_plan_run walks ops
 * [first, last) in ONE call — the reference drives its layers from Python one nn.Module at a time (yolact.py:564-676); ~230
 * interpreter-level calls per batch-8 step is what that shape costs here, and on a slow host it bounds batch 1.
 * Descriptors are caller-owned and may be patched between runs (input pointer, prototype output).  `events`: handles from
 * ymi_event_create, indexed by RECORD / WAIT ops.  overlap = 0: everything on stream_a, markers skipped (serialised kernels, what
 * per-kernel timing needs).  skip_sections: bit k set = ops whose `section` is k are skipped (bit YMI_SEC_PROTO: the protonet, when
 * cfg.eval_mask_branch is False).  On failure returns the failing call's code and, through failed_op, its index. */
enum { YMI_OP_NOP = 0, YMI_OP_CONV = 1, YMI_OP_WINO = 2, YMI_OP_DCN = 3, YMI_OP_CHAIN = 4, YMI_OP_STEM = 5, YMI_OP_INPUT = 6,
       YMI_OP_BILINEAR = 7, YMI_OP_MAXPOOL = 8, YMI_OP_BILINEAR_ADD = 9, YMI_OP_RECORD = 10, YMI_OP_WAIT = 11, YMI_OP_MEMSET = 12,
       YMI_OP_STAGE_EXIT = 13 };
enum { YMI_SEC_NONE = 0, YMI_SEC_BACKBONE = 1, YMI_SEC_FPN = 2, YMI_SEC_PROTO = 3, YMI_SEC_HEADS = 4 };
typedef struct ymi_plan_op {
  int32_t kind;        /* YMI_OP_* */
  int32_t stream;      /* 0 = A, 1 = B */
  int32_t section;     /* YMI_SEC_* (the reference's timer sections, yolact.py:570-607) */
  int32_t _pad;
  const void *desc;    /* CONV / WINO / DCN / CHAIN / STEM / STAGE_EXIT: the call's descriptor */
  void *p[3];          /* pointer arguments of the descriptor-less calls (see csrc/plan_exec.cpp) */
  int64_t i[8];        /* their integer arguments; RECORD / WAIT: i[0] = event index; MEMSET: i[0] = bytes */
  double f[2];         /* BILINEAR: scale_h, scale_w */
} ymi_plan_op;
int ymi_event_create(void **ev);
int ymi_event_destroy(void *ev);
int ymi_plan_run(const ymi_plan_op *ops, int first, int last, void *stream_a, void *stream_b, void *const *events, int overlap,
                 int skip_sections, int32_t *failed_op);

/* -- workspace sizes (ABI 7) ------------------------------------------------------------------------------------------------
 * The library never allocates device memory (SURVEY 8(b) "ownership": the reference's extension allocates its own outputs and
 * scratch, dcn_v2_cuda.cu:89-91,165-170; here the CALLER does).  A host that is not the Python shim asks this function how many
 * BYTES a workspace needs instead of re-deriving the formulas in the comments above.  `what` selects the workspace, `desc` points
 * at the descriptor of the call it belongs to (only shape fields are read, pointers may be NULL).  Returns the size in bytes
 * (>= 0; 0 = the call needs no such workspace in this configuration) or a negative YMI_E* code. */
enum {
  YMI_WS_WINO_V = 1,        /* desc: ymi_wino_desc      -> ymi_wino_desc.V  = G*T*C floats, T = B*ceil(H/m)*ceil(W/m) (nlev > 0: summed over lev[]), G = (m+2)^2 */
  YMI_WS_WINO_M = 2,        /* desc: ymi_wino_desc      -> ymi_wino_desc.M  = G*T*ceil(Cout/4)*4 floats */
  YMI_WS_SPLITK = 3,        /* desc: ymi_conv_desc      -> ymi_conv_desc.split_ws = split_k * B*Ho*Wo * Cout floats (0 when split_k <= 1) */
  YMI_WS_MASK_IOU = 4,      /* desc: ymi_mask_iou_shape -> ymi_mask_iou_f32's ws = A*B + A + B floats */
  YMI_WS_JPEG_COEFS = 5,    /* desc: ymi_jpeg_info filled by ymi_jpeg_parse -> int16 coefficient buffer (host, and its device copy) */
  YMI_WS_JPEG_PLANES = 6,   /* desc: ymi_jpeg_info      -> ymi_jpeg_reconstruct_bgr_u8's planes_ws */
  YMI_WS_DETECT_SCORES_T = 7,   /* desc: ymi_detect_desc -> scores_t  [B,C-1,P] floats */
  YMI_WS_DETECT_PER_PRIOR = 8,  /* desc: ymi_detect_desc -> keep / maxsc / argmax: [B,P] 4-byte elements EACH */
  YMI_WS_DETECT_CAND = 9,       /* desc: ymi_detect_desc -> cand_score / cand_prior: [B,(C-1)*top_k] 4-byte elements EACH */
  YMI_WS_DETECT_REC = 10,       /* desc: ymi_detect_desc -> out_rec [B, 1 + cap*(6+D)] floats, cap = cross_class ? top_k : max_det */
  YMI_WS_AMAX_SLOT = 11,        /* desc: NULL            -> one magnitude-bound slot (x_amax / y_amax): YMI_AMAX_SUB * YMI_AMAX_STRIDE floats */
  YMI_WS_RLE_COUNTS = 12,       /* desc: ymi_rle_shape   -> ymi_mask_rle_f32's counts [N,cap] uint32 (cap = h*w + 1 covers every mask) */
  YMI_WS_DETECT_GREEDY = 13,    /* desc: ymi_detect_desc -> ymi_detect_greedy_ws.ws: boxes [B,P,4] floats, survivor keys / priors
                                 * [B,(C-1)*max_det] 8 + 4 bytes, large-K candidate keys [B,C-1,P] 8 bytes; each part 256-byte aligned */
  YMI_WS_JPEG_ENC = 14,         /* desc: ymi_jpeg_enc_desc, h / w / subsampling read -> ymi_jpeg_enc_desc.ws */
  YMI_WS_JPEG_ENC_OUT = 15,     /* desc: ymi_jpeg_enc_desc, same fields -> least ymi_jpeg_enc_desc.out_capacity: an upper bound of
                                 * the stuffed scan + EOI for ANY pixels (416 bytes per coded 8x8 block + 2) */
  YMI_WS_MASK_LOSS = 16,        /* desc: ymi_mask_loss_desc, mh / mw / N read -> ymi_mask_loss_desc.ws: per-tile partial sums of
                                 * d_coef and L_j, ceil(mh*mw / 256) * N * 33 + N floats (+ 256 bytes: never empty) */
  YMI_WS_MATCH = 17,            /* desc: ymi_match_desc, B / P / G read -> ymi_match_desc.ws: per tile and GT the best (overlap,
                                 * prior), per image and prior the best (overlap, GT), crowd ratio and forced GT, row state, per-tile
                                 * counts and sums: 4 * (2 T G + 4 B P + 2 G + 2 B T) bytes, T = ceil(P / 256), each part padded to 16 */
  YMI_WS_BOX_LOSS = 18,         /* desc: ymi_match_desc, B / P read -> ymi_box_loss_f32's ws: 2 * 4 B T bytes, each part padded to 16 */
  YMI_WS_CLASS_LOSS = 19,       /* desc: ymi_class_loss_desc, B / P / C read -> ymi_class_loss_desc.ws: per prior the mining key and lse,
                                 * per tile the positives and the loss partial: 4 * (2 B P + 2 B T) bytes, T = ceil(P / R),
                                 * R = min(128, 10752 / (C | 1)) rows per tile, each part padded to 16 */
  YMI_WS_SEGM_LOSS = 20,        /* desc: ymi_segm_loss_desc, B / mh / mw read -> ymi_segm_loss_desc.ws: 4 B ceil(mh*mw / 256) bytes,
                                 * padded to 16 */
  YMI_WS_MASKIOU_INPUT = 21,    /* desc: ymi_maskiou_input_desc, mh / mw / N read -> its ws: ceil(mh*mw / 256) * N * 32 floats */
  YMI_WS_CONV_BWD = 22,         /* desc: ymi_conv_bwd_desc, the shape read -> its ws: chunks * (kh*kw*Cin + 1) * ceil4(Cout) floats */
  YMI_WS_MASKIOU_HEAD = 23,     /* desc: ymi_maskiou_head_desc, N read -> its ws: N floats, padded to 16 */
  YMI_WS_CONV_WGRAD = 24,       /* desc: ymi_conv_wgrad_desc, the shape read -> its ws: chunks * kh*kw*Cin * Cout floats and chunks *
                                 * Cout floats, each part padded to 16 */
  YMI_WS_BN = 25,               /* desc: ymi_bn_desc, npos / C read -> its ws: 2 * chunks * C + 2 * C floats, chunks = ceil(npos / max(32,
                                 * ceil(npos / 1024))), each part padded to 16 */
  YMI_WS_STEM_WGRAD = 26,       /* desc: ymi_stem_wgrad_desc, the shape read -> its ws: chunks * 147 * Cout floats, padded to 16 */
  YMI_WS_AUGMENT = 27,          /* desc: ymi_augment_desc, B / n_masks read -> its ws: B records, n_masks (image, instance) pairs and B
                                 * pairs of resize scales, B * sizeof(ymi_augment_rec) + 8 n_masks + 16 B bytes, each part padded to 16 */
  YMI_WS_PRECONV_WGRAD = 28,    /* desc: ymi_preconv_wgrad_desc, the shape read -> its ws: chunks * 27 * Cout floats, padded to 16 */
  YMI_WS_CONV_WGRAD_H2 = 29,    /* desc: ymi_conv_wgrad_desc, the shape read -> ymi_conv_wgrad_nhwc_h2's ws: the two parts of
                                 * YMI_WS_CONV_WGRAD, then kh*kw * chunks * per + 64 and chunks * per + 64 table entries (per = the
                                 * positions of a chunk) and 2048 partial bounds, 4 bytes each, each part padded to 16 */
  YMI_WS_COCO_MASK = 30         /* desc: ymi_coco_mask_desc, n / n_vert / n_poly / n_counts read -> its ws: 16 n_vert +
                                 * n * sizeof(ymi_coco_mask_rec) + 4 n_poly + 4 n_counts bytes, each part padded to 16 */
};
typedef struct { int32_t A, B; int64_t n; } ymi_mask_iou_shape;
typedef struct { int32_t N, h, w, cap; } ymi_rle_shape;      /* cap <= 0: the safe capacity h*w + 1 */
int64_t ymi_workspace_bytes(int what, const void *desc);

/* -- the SGD update (csrc/sgd.hip; additive to ABI 9) ------------------------------------------------------------------------------
 * train.py:215-216,316-318: torch.optim.SGD(lr, momentum, weight_decay).step() behind `if torch.isfinite(loss).item()`, and
 * optimizer.zero_grad(), over EVERY tensor of a parameter group in ONE launch with no host read.  Per element, every operation rounded
 * once to fp32 (no FMA contraction), so numpy fp32 restates it bit for bit:
 *     d = g + wd * p              (wd == 0: d = g exactly)
 *     m = mom * m + d             (the buffers start at zero, so the first step gives m = d, as torch does)
 *     p = p - lr * m              (mom == 0: p = p - lr * d and m is neither read nor written)
 * Dampening and Nesterov are not offered.  These are NOT torch's bits: torch's foreach / fused kernels contract to FMAs.
 * Guard: with `loss` given and *loss not finite, no p and no m changes and one thread adds 1 to *skipped (a plain load and store).
 * With zero_grad the gradients are zeroed in the same pass, applied or skipped.
 * tensors [n_tensors] and chunks [n_chunks] are DEVICE tables; a chunk is up to YMI_SGD_CHUNK elements of one tensor starting at
 * `first` (a multiple of YMI_SGD_CHUNK: ymi_sgd_plan writes the table).  One block walks a chunk; the grid is min(n_chunks,
 * max_blocks) blocks, which stride over the chunks (max_blocks 0: 2048).  A chunk whose p, g and m are 16-byte aligned moves as
 * 16-byte loads and stores with a scalar tail, any other one element at a time.  A chunk record that points outside its tensor, or
 * outside the tensor table, is passed over.  No atomics, no LDS, bit-reproducible.
 * YMI_ENULL: the descriptor NULL.  YMI_EARG: tensors or chunks NULL, n_tensors / n_chunks / max_blocks < 0, momentum < 0 or not
 * finite; and, where the optional HOST copy of the tensor table `tensors_host` is given: p or g NULL, n < 0, m NULL with
 * momentum > 0 (without the host copy the kernel leaves such a tensor untouched). */
#define YMI_SGD_CHUNK 4096           /* elements; a multiple of 4 */
typedef struct { float *p, *g, *m; int64_t n; } ymi_sgd_tensor;
typedef struct { int32_t tensor; int32_t _pad0; int64_t first; } ymi_sgd_chunk;
typedef struct {
  const ymi_sgd_tensor *tensors;       /* device [n_tensors] */
  const ymi_sgd_chunk *chunks;         /* device [n_chunks] */
  const ymi_sgd_tensor *tensors_host;  /* host copy of `tensors` to validate, or NULL */
  const float *loss;                   /* device scalar the guard reads, or NULL: always apply */
  int32_t *skipped;                    /* device counter of skipped steps, or NULL */
  int32_t n_tensors, n_chunks;
  float lr, momentum, weight_decay;    /* rounded to fp32 once, by the caller */
  int32_t zero_grad;                   /* != 0: g = 0 in the same pass */
  int32_t max_blocks;                  /* 0: the default cap of 2048 blocks */
  int32_t _pad0;
} ymi_sgd_desc;
int ymi_sgd_step_f32(const ymi_sgd_desc *d, void *stream);
/* HOST.  The chunk table of tensors of numel[0 .. n) elements, tensor by tensor, a tensor of 0 elements getting none; returns its
 * length, and writes its first min(length, cap) records to `out` unless `out` is NULL.  YMI_EARG: numel NULL with n > 0, n < 0, a
 * negative numel, cap < 0. */
int64_t ymi_sgd_plan(const int64_t *numel, int n, ymi_sgd_chunk *out, int64_t cap);

/* -- box calibration (ABI 7; csrc/calib.hip) ------------------------------------------------------------------------------------
 * Two fixed micro-workloads the caller times (events on `stream`) right before a benchmark, so that a throughput number can be
 * attributed to the box or to the code (bench.py `box_calibration`).  Not on the product path.
 * ymi_calib_mfma_f16: `blocks` x 4 waves, each `iters` x 4 register-resident v_mfma_f32_32x32x16_f16 on random-mantissa operands;
 *   *flops = the fp16 FLOPs executed.  ymi_calib_hbm_copy: dst[i] = src[i] over n_floats (n % 4 == 0, 16-byte aligned), float4
 *   lanes; *bytes = read + written. */
int ymi_calib_mfma_f16(float *out, int blocks, int iters, double *flops, void *stream);
int ymi_calib_hbm_copy(const float *src, float *dst, long n_floats, double *bytes, void *stream);
/* every one of `blocks` 256-thread blocks reads src [n_floats] (n % 4096 == 0; 1 MB stays resident in every XCD's L2) `iters` times with
 * 16-byte loads; *bytes = bytes delivered to the CUs.  The path the GEMM tiles are bound by (global -> CU at L2-hit latency). */
int ymi_calib_l2_read(const float *src, long n_floats, int blocks, int iters, float *out, double *bytes, void *stream);
/* one lane follows i = chain[i] from `start` for `hops` dependent loads and stores where it ended in out[0]; the caller lays the
 * permutation (one entry per 128-byte line over the footprint to probe) and divides its event time by hops: load-to-use latency. */
int ymi_calib_latency(const int32_t *chain, long n, int start, int hops, int32_t *out, void *stream);

/* -- the train-mode DarkNet53 backbone (csrc/bn_train.hip, csrc/darknet_train.hip; additive, the ABI number stays) ----------------------
 * backbone.py:222-294: every layer is a bias-free convolution, BatchNorm2d, LeakyReLU(0.1); a DarkNetBlock is conv2(conv1(x)) + x.  The
 * convolutions of 32 .. 1024 input channels run on ymi_conv2d_nhwc_f32 / ymi_conv_wgrad_nhwc_f32 / ymi_conv_dgrad_s2_nhwc_f32; the
 * pre-convolution's forward is ymi_conv2d_nhwc_f32 with Cin = 4.  No atomics; every element of every output is written exactly once;
 * the same inputs give the same bits.
 *
 * ymi_bn_leaky_fwd_nhwc_f32 / ymi_bn_leaky_bwd_nhwc_f32: ymi_bn_fwd_nhwc_f32 / ymi_bn_bwd_nhwc_f32 (same descriptor, same workspace, same
 * statistics, mean / invstd, running update, two-pass variance and COLUMN SUMS) with LeakyReLU(0.1) and the residual BEHIND it:
 *     z = gamma (x - mean) invstd + beta;  a = z > 0 ? z : 0.1f * z (one fp32 multiply);  y = a + res, or a when res is NULL
 *     gh = z > 0 ? dy : 0.1f * dy;  dbeta, dgamma and dx from gh by ymi_bn_bwd_nhwc_f32's formulas, chunks and order of additions.
 * d_res is dy itself: no kernel writes it, and d->d_res must be NULL.  d->relu must be 0.
 * THE SLOPE DECISION z > 0 is made once, by the forward.  Without a residual y > 0 is exactly z > 0 and the backward reads it from
 * d->y (pass mask = NULL to both).  With a residual the forward writes it to `mask`, ceil(npos C / 32) uint32 words, 16-byte aligned: bit
 * (i & 31) of word i >> 5 belongs to element i of the [npos, C] map, the bits past the last element are 0, every word is written exactly
 * once.  The backward given that mask reads the bit (and not d->y); z is never computed a second time.  The forward writes a mask
 * whenever one is given.  With gamma = beta = 0 every z is 0 and gh is 0.1f * dy, as in PyTorch.
 * Errors as for the plain pair, and: YMI_EARG: relu != 0, d_res != NULL (backward); YMI_ENULL: res without a mask (forward), neither a
 * mask nor y (backward); YMI_ESHAPE: a mask not 16-byte aligned.  No error path launches anything. */
int ymi_bn_leaky_fwd_nhwc_f32(const ymi_bn_desc *d, uint32_t *mask, void *stream);
int ymi_bn_leaky_bwd_nhwc_f32(const ymi_bn_desc *d, const uint32_t *mask, void *stream);

/* ymi_preconv_wgrad_nhwc_f32: dw[k,co] = sum_pos x[n, oy + ky - 1, ox + kx - 1, ci] g[pos,co], k = (ky*3 + kx)*3 + ci (27 rows),
 * pos = [n, oy, ox] over the B H W positions of g (3x3 / stride 1 / pad 1), any H, W >= 1, reads outside the image are 0.  x is the
 * NHWC-4 image the forward's Cin-4 loader reads; its channel 3 is padding, is never addressed and reaches no row of dw WHATEVER IT
 * HOLDS; taps outside the image and positions past a chunk are masked by a select, never by a product.  On v_mfma_f32_32x32x2_f32
 * (fp32 in, fp32 accumulate) with the positions as its k index and the 27 rows as rows 0 .. 26 of one 32-row tile.  No data gradient:
 * nothing upstream of the image needs one.
 * SUMMATION ORDER (part of the contract, a function of the shape only): the positions n-major, then oy, then ox, are cut into chunks of
 * per = 32 ceil(ceil(P / 32) / min(ceil(P / 32), ceil(2048 / (Cout / 32)))) positions, P = B H W.  A chunk's partial sum starts from
 * +0.0 and takes its positions in ascending order two at a time: one instruction adds the two products of positions p and p + 1
 * (p - chunk start even; a tap outside the image or a position past the chunk contributes an exact 0 product).  The partials go to ws
 * and a second launch adds them in chunk order from +0.0.
 * YMI_ENULL: the descriptor, x, g, dw or ws NULL; YMI_EARG: B, H, W or Cout < 1; YMI_ESHAPE: Cout % 32, ldg < Cout, ldg % 4, x or g of
 * 2^29 elements or more, ws not 16-byte aligned, ws_bytes too small.  No error path launches anything. */
typedef struct ymi_preconv_wgrad_desc {
  const float *x;               /* [B,H,W,4] */
  const float *g;               /* [B,H,W,ldg], channels [0, Cout) are read */
  float *dw;                    /* [27, Cout] */
  void *ws;                     /* ymi_workspace_bytes(YMI_WS_PRECONV_WGRAD, desc) bytes, 16-byte aligned */
  int64_t ws_bytes;
  int32_t B, H, W, Cout, ldg, _pad0;
} ymi_preconv_wgrad_desc;
int ymi_preconv_wgrad_nhwc_f32(const ymi_preconv_wgrad_desc *d, void *stream);

/* -- profiling hooks -------------------------------------------------------------------- */
/* When enabled, every conv launch is bracketed by hipEvents on its stream; ymi_prof_read returns
 * (after synchronising) per-launch milliseconds, flops and tile ids. Used by bench.py roofline. */
/* Diagnostics: when buf != NULL every conv block writes 8 x uint64 {xcc<<32 | HW_ID, t_start, t_loop, t_epilogue, t_end,
 * t_transposed, t_computed, 0} (shader clock) at buf[blockIdx*8]; cap_blocks = capacity in blocks (larger grids are not traced). NULL disables. */
int ymi_debug_set_trace(void *buf, long cap_blocks);
int ymi_prof_enable(int on);
int ymi_prof_count(void);
int ymi_prof_read(int i, float *ms, double *flops, int32_t *tile, int32_t *kind);
int ymi_prof_reset(void);

#ifdef __cplusplus
}
#endif
#endif
