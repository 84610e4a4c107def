// The tail of one ResNet bottleneck and the head of the next in ONE streaming launch (backbone.py:37-57, first stage: planes = 64):
//     y = relu(bn3(conv3 1x1 (64 -> 256)(t)) + residual)          Bottleneck.forward of block b, lines 3..5 from the end
//     z = relu(bn1(conv1 1x1 (256 -> 64)(y)))                      Bottleneck.forward of block b + 1, first line
// At 138 x 138 x 8 both layers are pure streams (5 GFLOP each against 351 / 195 MB): conv3 reads t (39 MB) and the residual
// (156 MB) and writes y (156 MB); conv1 reads y back and writes z (39 MB).  In the plan they took 0.083 + 0.055 ms, i.e. 4.2 and
// 3.5 TB/s; here y is read back from LDS, not from memory, and the launch is one pass of 390 MB.
//
// One block per CU, persistent, 8 waves.  Every wave keeps ITS filters in registers for the launch's lifetime, as MFMA operand
// fragments (96 VGPRs: 32 channels of conv3, 16 channels x K = 256 of conv1) — the first version kept both filter sets in LDS
// (141 KB) and spent its time on 52 ds_read_b128 per wave per 16 pixels (profiles/r04_chain_probe.txt, first table: 0.100 ms).
// Per iteration the block takes 32 pixels:
//   P1  t tile (32 x 64 fp32, requested one iteration ahead) -> two fp16 planes in LDS (tensor scale from x_amax)        | barrier
//   P2  GEMM 1 on v_mfma_f32_16x16x32_f16, issued as W X^T: wave w owns output channels 32 w .. 32 w + 31 of both 16-pixel
//       halves; a lane ends with four consecutive channels of one pixel
//   P3  epilogue 1 in that layout: scale / bias / + residual (float4, requested one iteration ahead) / ReLU / float4 store of y;
//       the wave's two 16 x 32 slices of y -> fp16 planes in LDS, each with the power-of-two scale of ITS OWN maximum     | barrier
//   P4  GEMM 2: wave (q, i) owns z channels 16 q .. + 15 of half i; the K = 256 sum is taken slice by slice (32 channels = one
//       producing wave), each partial sum divided by its slice's scale (exact): no block- or tensor-wide bound of y is needed
//   P5  epilogue 2: scale / bias / ReLU / float4 store of z
// ONE LDS-only barrier per 32 pixels (operand tiles double-buffered; P4 / P5 of tile k - 1 run next to P2 / P3 of tile k); the
// global loads of iteration i + 1 are in flight during iteration i; all memory
// operations are unconditional buffer operations (out-of-range offsets for masked rows), so the compiler's vmcnt is exact.
// Magnitude bounds of y and z are reported like every other launch (ymi_amax_*).  z == nullptr: GEMM 2 is skipped (conv3 alone:
// the last block of the stage, whose consumer is not a 64-channel 1x1).
#include "gemm_h2.h"
#include <type_traits>

int ymi_internal_prof_begin(double flops, int tile, int kind, hipStream_t s);
void ymi_internal_prof_end(int idx, hipStream_t s);

namespace {

using namespace ymi_h2;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int K1 = 64, N1 = 256, PX = 32, NW = 8;
constexpr int RS1 = 2 * K1 + 16;          // bytes per LDS row of a K = 64 plane (128 + 16: the 16 lanes of a read phase hit 16 bank groups)
constexpr int RS2 = 2 * N1 + 16;          // ... of a K = 256 plane
constexpr int A1_PLANE = PX * RS1, A2_PLANE = PX * RS2;
// LDS: the two operand tiles and the slice scales are DOUBLE-buffered (iteration k works in buffer k & 1), which is what lets one
// barrier per iteration do (see the kernel): 2 x 9.2 KB + 2 x 33.8 KB + scales + conv3's per-lane epilogue constants
constexpr int A1_BUF = 2 * A1_PLANE, A2_BUF = 2 * A2_PLANE;
constexpr int OFF_A1 = 0, OFF_A2 = OFF_A1 + 2 * A1_BUF, OFF_SC = OFF_A2 + 2 * A2_BUF, OFF_EP = OFF_SC + 2 * (2 * NW * 4),
              CH_LDS = OFF_EP + NW * 2 * 4 * 32;   // OFF_EP: conv3's per-lane epilogue constants (scale, bias) x (wave, j, g)
// N2 = 128 (the stage exit, see below): the second layer's per-lane epilogue constants live in LDS too, (scale, bias) x (wave, tt, g)
// and so does the LOW plane of its filters (64 KB, in fragment order: 1 KB = the 64 lanes' 16 bytes of one (16-channel tile,
// 32-deep chunk), conflict-free ds_read_b128): with both planes in registers the kernel needs 256 VGPRs + 156 bytes of scratch
constexpr int OFF_EP2 = CH_LDS, OFF_WL = OFF_EP2 + NW * 2 * 4 * 32, CH_LDS_X = OFF_WL + 128 * N1 * 2;
static_assert(CH_LDS_X <= 160 * 1024, "LDS of a CU");
// ENTRY (the stage's first block, see below): a second double-buffered K = 64 tile — the block input x0, the operand of the projection
// shortcut — and the shortcut's per-lane epilogue constants, (scale, bias) x (wave, j, g) like conv3's
// and the LOW plane of the shortcut's filters (32 KB, fragment order as OFF_WL above: 1 KB = the 64 lanes' 16 bytes of one (wave, j, c);
// every lane reads back what it wrote itself): with both planes in registers the kernel needs 256 VGPRs + 60 bytes of scratch
constexpr int OFF_A0 = CH_LDS, OFF_EPD = OFF_A0 + 2 * A1_BUF, OFF_WDL = OFF_EPD + NW * 2 * 4 * 32, CH_LDS_E = OFF_WDL + N1 * K1 * 2;
static_assert(CH_LDS_E <= 160 * 1024, "LDS of a CU");

struct ChainParams {
  const float *x, *res, *x_amax;
  const void *wa, *wb;                    // fp16 planes [2][cpa][64] / [2][cpb][256]
  const float *sa, *ba, *sb, *bb;         // scale_h2 / bias of the two layers
  float *y, *z, *y_amax, *z_amax;
  int M, ldx, res_ld, ldy, ldz, act_a, act_b;
  unsigned wa_plane, wb_plane;            // bytes per plane
};
// N2 = 128 (a type of its own: the 64-wide kernel keeps its kernel-argument layout, hence its code): y is stored only at pixels with
// h % y_stride == 0 && w % y_stride == 0 (M == B H W); mag_w / mag_h = ceil(2^32 / W), ceil(2^32 / H): m / W == (m * mag_w) >> 32
// exactly for every m with m * W < 2^32 (the error term is m * (W * mag_w - 2^32) / (W * 2^32) < m / 2^32, which must stay below
// 1 / W), and (m / W) / H likewise while (m / W) * H < 2^32: the entry point refuses shapes with M * max(H, W) >= 2^32
struct ChainParamsX : ChainParams {
  unsigned long long mag_w, mag_h;
  int H, W, y_stride;
};
// ENTRY (again a type of its own): the block input x0 [M, ldx0] with its magnitude slot, the shortcut's fp16 planes [2][cpd][64],
// scale_h2 and bias
struct ChainParamsE : ChainParams {
  const float *x0, *x0_amax;
  const void *wd;
  const float *sd, *bd;
  int ldx0;
  unsigned wd_plane;
};
template <int N2, bool ENTRY>
using chain_params_t = std::conditional_t<ENTRY, ChainParamsE, std::conditional_t<N2 == 128, ChainParamsX, ChainParams>>;

// N2 = the second layer's width.  64: the pair inside the stage (above; this instantiation's ISA is the untemplated kernel's,
// instruction for instruction).  128: the stage EXIT, layer0.2.conv3 -> layer1.0.conv1 (256 -> 128, ymi_stage_exit_chain_f32): wave
// (q, i) owns z channels 32 q .. 32 q + 31 of half i — NT = 2 sixteen-channel tiles that share the y fragments read from LDS (48
// MFMAs per wave per tile in GEMM 2 instead of 24, the reads of the y planes unchanged) — and y is stored only where the stride-2
// projection shortcut of the next stage reads it (ChainParamsX::y_stride; the bound y_amax still covers EVERY pixel, so that
// launch's fp16x2 scale, hence its output, does not move).  Same loop: per-slice scales, one barrier per iteration, two buffers,
// unconditional buffer operations.
// Registers (8 waves per CU = 2 per SIMD: 256 per lane; hipcc 7.2 -Rpass-analysis=kernel-resource-usage):
//     N2 =  64                                    246 VGPRs, 0 AGPRs, no scratch,  88 192 B of LDS
//     N2 = 128, both planes of conv1 in registers 256 VGPRs, 0 AGPRs, 156 B of scratch per lane      (not shipped)
//     N2 = 128, conv1's LOW plane in LDS          238 VGPRs, 0 AGPRs, no scratch, 155 776 B of LDS   (shipped)
// 32 + 128 filter registers fit on paper, but next to the two residual sets (32), the accumulators and the addresses the allocator
// spills 39 of them; the low plane (one of three products) costs 16 conflict-free ds_read_b128 per wave per 32 pixels instead.
//
// ENTRY (N2 = 64 only): the stage's FIRST block, layer0.0.conv3 -> layer0.1.conv1, whose residual is the projection shortcut
// r = bn_d(W_d x0) (1x1, 64 -> 256, no activation) of the block input x0.  r is computed HERE instead of being read: per iteration
// the block also takes its 32 x 64 tile of x0 (this thread's 16 bytes, requested one iteration ahead like t's), splits it into two
// fp16 planes with x0's OWN power-of-two scale (x0_amax) into a second double-buffered LDS tile, and a second accumulator set
// accd = W_d x0 runs on the same MFMA with the same three-product order as GEMM 1, one 16-pixel half at a time in front of the
// epilogue of that half.  The wave's 32 channels of W_d: the high plane as register fragments like conv3's, the low plane in LDS
// in fragment order (this form loads no residual, so the two residual sets' 32 VGPRs are free).  Epilogue 1 keeps its expression
// order with r = accd * (scale_d / s_x0) + bias_d in the residual's place, so against the two launches (shortcut, then chain) at
// most the summation order inside accd differs.  The 256-channel shortcut tensor is never written or read: 273 MB per batch-8
// launch against 195 + 390.  Registers (same remark as above; none of the other two instantiations' instructions move):
//     both planes in registers, all four accd tiles next to GEMM 1's   256 VGPRs, 60 B of scratch per lane          (not shipped)
//     low plane in LDS, all four accd tiles                            256 VGPRs, 12 B of scratch per lane          (not shipped)
//     low plane in LDS, accd half by half                              253 VGPRs, no scratch, 141 440 B of LDS      (shipped)
template <int N2, bool ENTRY = false>
__global__ __launch_bounds__(64 * NW) void chain_h2_k(const chain_params_t<N2, ENTRY> p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NT = N2 / 64;                          // 16-channel tiles of z per wave
  constexpr bool EXIT = N2 == 128;
  static_assert(!(ENTRY && EXIT), "the entry form is the 64-wide pair's");
  __shared__ __attribute__((aligned(16))) char lds[EXIT ? CH_LDS_X : ENTRY ? CH_LDS_E : CH_LDS];
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lr = lane & 15, g = lane >> 4;
  const int q2 = wave & 3, i2 = wave >> 2;             // GEMM 2: this wave's 16 z channels (16 q2 ..) and 16-pixel half of the tile
  float sA, invA;
  ymi_h2_scale(ymi_amax_read(p.x_amax), sA, invA);
  float sD = 1.f, invD = 1.f;                          // ENTRY: x0's scale, independent of t's
  if constexpr (ENTRY) ymi_h2_scale(ymi_amax_read(p.x0_amax), sD, invD);
  const ymi_amax_pre apre_y = ymi_amax_prefetch(p.y_amax);
  const ymi_amax_pre apre_z = ymi_amax_prefetch(p.z_amax);
  const bool two = p.z != nullptr;

  // ---- this wave's filters -> REGISTERS, once: as MFMA A-operand fragments (row = output channel lr of a 16-channel tile, 8
  // consecutive k at 8 g of a 32-deep chunk).  GEMM 1: channels 32 wave + 16 j + lr, chunks 0 / 1; GEMM 2: channels 16 q2 + lr, chunks 0 .. 7
  f16x8 w3h[2][2], w3l[2][2], w1h[NT][8], w1l[EXIT ? 1 : NT][EXIT ? 1 : 8];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const char *src = reinterpret_cast<const char *>(p.wa) + (size_t)(32 * wave + 16 * j + lr) * (2 * K1) + c * 64 + g * 16;
      w3h[j][c] = *reinterpret_cast<const f16x8 *>(src);
      w3l[j][c] = *reinterpret_cast<const f16x8 *>(src + p.wa_plane);
    }
  f16x8 wdh[ENTRY ? 2 : 1][ENTRY ? 2 : 1];           // ENTRY: the shortcut's, same channels, same fragments; the low plane -> LDS
  if constexpr (ENTRY) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const char *src = reinterpret_cast<const char *>(p.wd) + (size_t)(32 * wave + 16 * j + lr) * (2 * K1) + c * 64 + g * 16;
        wdh[j][c] = *reinterpret_cast<const f16x8 *>(src);
        *reinterpret_cast<f16x8 *>(lds + OFF_WDL + (((wave * 2 + j) * 2 + c) * 64 + lane) * 16) = *reinterpret_cast<const f16x8 *>(src + p.wd_plane);
      }
  }
#pragma unroll
  for (int tt = 0; tt < NT; ++tt)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const f16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
      const char *src = reinterpret_cast<const char *>(p.wb) + (size_t)(16 * NT * q2 + 16 * tt + lr) * (2 * N1) + c * 64 + g * 16;
      w1h[tt][c] = two ? *reinterpret_cast<const f16x8 *>(src) : z8;
      if constexpr (!EXIT) w1l[tt][c] = two ? *reinterpret_cast<const f16x8 *>(src + p.wb_plane) : z8;
    }
  if constexpr (EXIT) {                                // the low plane -> LDS, fragment order; published by the first iteration's barrier
#pragma unroll
    for (int k = 0; k < 8; ++k) {                      // chunk (tile16 = k, c = t >> 6, lane = t & 63)
      const int c = t >> 6;
      const char *src = reinterpret_cast<const char *>(p.wb) + p.wb_plane + (size_t)(16 * k + lr) * (2 * N1) + c * 64 + g * 16;
      const f16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
      *reinterpret_cast<f16x8 *>(lds + OFF_WL + ((k * 8 + c) * 64 + lane) * 16) = two ? *reinterpret_cast<const f16x8 *>(src) : z8;
    }
  }
  // per-lane epilogue constants: channels 32 wave + 16 j + 4 g .. + 3 of conv3, 16 q2 + 4 g .. + 3 of conv1
  // (conv3's live in LDS, 32 bytes per (wave, j, g), and are re-read in every epilogue: 16 registers the filter fragments need)
  if (lr == 0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = 32 * wave + 16 * j + 4 * g;
      f32x4 sc, bi;
#pragma unroll
      for (int e = 0; e < 4; ++e) { sc[e] = p.sa[n + e] * invA; bi[e] = p.ba ? p.ba[n + e] : 0.f; }
      *reinterpret_cast<f32x4 *>(lds + OFF_EP + ((wave * 2 + j) * 4 + g) * 32) = sc;
      *reinterpret_cast<f32x4 *>(lds + OFF_EP + ((wave * 2 + j) * 4 + g) * 32 + 16) = bi;
      if constexpr (ENTRY) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { sc[e] = p.sd[n + e] * invD; bi[e] = p.bd ? p.bd[n + e] : 0.f; }
        *reinterpret_cast<f32x4 *>(lds + OFF_EPD + ((wave * 2 + j) * 4 + g) * 32) = sc;
        *reinterpret_cast<f32x4 *>(lds + OFF_EPD + ((wave * 2 + j) * 4 + g) * 32 + 16) = bi;
      }
    }
  }
  f32x4 sc1 = {1.f, 1.f, 1.f, 1.f}, bi1 = {0.f, 0.f, 0.f, 0.f};
  if constexpr (EXIT) {                                // (the registers belong to the filter fragments: constants in LDS, as conv3's)
    if (lr == 0) {
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const int n = 16 * NT * q2 + 16 * tt + 4 * g;
        f32x4 sc = sc1, bi = bi1;
        if (two) {
#pragma unroll
          for (int e = 0; e < 4; ++e) { sc[e] = p.sb[n + e]; bi[e] = p.bb ? p.bb[n + e] : 0.f; }
        }
        *reinterpret_cast<f32x4 *>(lds + OFF_EP2 + ((wave * 2 + tt) * 4 + g) * 32) = sc;
        *reinterpret_cast<f32x4 *>(lds + OFF_EP2 + ((wave * 2 + tt) * 4 + g) * 32 + 16) = bi;
      }
    }
  } else if (two) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { sc1[e] = p.sb[16 * q2 + 4 * g + e]; bi1[e] = p.bb ? p.bb[16 * q2 + 4 * g + e] : 0.f; }
  }
  const float slope_a = ymi_act_slope(p.act_a);
  const float slope_b = ymi_act_slope(p.act_b);

  const int ntiles = (p.M + PX - 1) / PX;
  // loads of a tile: this thread's 16 bytes of t (pixel t >> 4 of 32, channels 4 (t & 15) ..), this lane's residual vectors (pixel
  // 16 i + lr, channels 32 wave + 16 j + 4 g ..).  Buffer loads / stores with an out-of-range offset for rows past M (and tiles
  // past the last): zeros back, nothing written, and NO branch — with conditional memory operations the compiler cannot count what
  // is outstanding and falls back to vmcnt(0) between iterations, i.e. it waits for the stores of y it has just issued
  const __amdgpu_buffer_rsrc_t xrs = buf_rsrc(p.x, (unsigned)p.M * (unsigned)p.ldx * 4u);
  const __amdgpu_buffer_rsrc_t rrs = buf_rsrc(p.res ? p.res : p.x, p.res ? (int)((unsigned)p.M * (unsigned)p.res_ld * 4u) : 0);
  const __amdgpu_buffer_rsrc_t yrs = buf_rsrc(p.y, (unsigned)p.M * (unsigned)p.ldy * 4u);
  const __amdgpu_buffer_rsrc_t zrs = buf_rsrc(p.z ? p.z : p.y, p.z ? (int)((unsigned)p.M * (unsigned)p.ldz * 4u) : 0);
  const int xp = t >> 4, xc = t & 15;
  auto load_x = [&](int tile) {
    const int m = tile * PX + xp;
    const unsigned off = (tile < ntiles && m < p.M) ? (unsigned)(m * p.ldx + 4 * xc) * 4u : OOB;
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, off, 0, 0));
  };
  // ENTRY: this thread's 16 bytes of x0, same pixel and channels as its 16 bytes of t (row pitch ldx0; only channels 0 .. 63 are read)
  __amdgpu_buffer_rsrc_t x0rs = xrs;
  if constexpr (ENTRY) x0rs = buf_rsrc(p.x0, (unsigned)p.M * (unsigned)p.ldx0 * 4u);
  auto load_x0 = [&](int tile) {
    if constexpr (ENTRY) {
      const int m = tile * PX + xp;
      const unsigned off = (tile < ntiles && m < p.M) ? (unsigned)(m * p.ldx0 + 4 * xc) * 4u : OOB;
      return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x0rs, off, 0, 0));
    } else {
      return f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto load_res = [&](int tile, f32x4 (&r)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = tile * PX + 16 * i + lr;
      const unsigned off = (tile < ntiles && m < p.M) ? (unsigned)(m * p.res_ld + 32 * wave + 4 * g) * 4u : OOB;
#pragma unroll
      for (int j = 0; j < 2; ++j) r[i][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrs, off + 64u * j, 0, 0));
    }
  };

  // LDS-only barrier: __syncthreads() would also wait for the global loads of the NEXT iteration (vmcnt(0)), i.e. expose one memory
  // round trip per tile
  // One iteration = 32 pixels, ONE barrier, software-pipelined over two tiles: after the barrier of iteration k the waves run
  // GEMM 2 + epilogue 2 of tile k - 1 (operands in buffer (k - 1) & 1, published by that barrier) and GEMM 1 + epilogue 1 of tile k
  // (t tile in buffer k & 1, written before the barrier) — two independent instruction streams for the scheduler, and half the
  // barriers of the first version.  Buffer k & 1 is next written in iteration k + 2, after every wave has passed barrier k + 1,
  // i.e. finished reading it.
  // `rv`: this tile's residual vectors (requested an iteration ago), `rn`: the registers the next tile's are requested into.  The
  // loop runs two iterations per trip with the two register sets (and the two LDS buffers) swapped: a copy rn -> rv at the end of
  // an iteration would wait for every outstanding memory operation, the stores of y just issued included (seen in the ISA as
  // s_waitcnt vmcnt(0) on the back edge).  Iterations past the last tile load nothing and store nothing but the last tile's z.
  float am_y = 0.f, am_z = 0.f;
  f32x4 xv, x0v;
  const int grid = (int)gridDim.x;
  auto iteration = [&](const int tile, auto buf_c, f32x4 (&rv)[2][2], f32x4 (&rn)[2][2]) {
    constexpr int BUF = decltype(buf_c)::value;
    char *const a1 = lds + OFF_A1 + BUF * A1_BUF;
    char *const a0 = lds + OFF_A0 + BUF * A1_BUF;       // (ENTRY only)
    char *const a2w = lds + OFF_A2 + BUF * A2_BUF;
    const char *const a2r = lds + OFF_A2 + (BUF ^ 1) * A2_BUF;
    float *const scw = reinterpret_cast<float *>(lds + OFF_SC) + BUF * (2 * NW);
    const float *const scr = reinterpret_cast<const float *>(lds + OFF_SC) + (BUF ^ 1) * (2 * NW);
    // P1: t tile -> planes
    {
      const f32x4 v = xv * sA;
      f16x4 h4, l4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const _Float16 h = (_Float16)v[e];
        h4[e] = h;
        l4[e] = (_Float16)(v[e] - (float)h);
      }
      char *dst = a1 + xp * RS1 + xc * 8;
      *reinterpret_cast<f16x4 *>(dst) = h4;
      *reinterpret_cast<f16x4 *>(dst + A1_PLANE) = l4;
    }
    if constexpr (ENTRY) {                              // ... and the x0 tile, with its own scale
      const f32x4 v = x0v * sD;
      f16x4 h4, l4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const _Float16 h = (_Float16)v[e];
        h4[e] = h;
        l4[e] = (_Float16)(v[e] - (float)h);
      }
      char *dst = a0 + xp * RS1 + xc * 8;
      *reinterpret_cast<f16x4 *>(dst) = h4;
      *reinterpret_cast<f16x4 *>(dst + A1_PLANE) = l4;
    }
    xv = load_x(tile + grid);                           // next iteration's operands: in flight until its P1 / P3
    if constexpr (ENTRY) x0v = load_x0(tile + grid);
    else load_res(tile + grid, rn);
    YMI_BARRIER();
    if (two) {
      // P4 (tile k - 1): GEMM 2 for pixels 16 i2 + lr, z channels 16 q2 ..: the K = 256 sum one 32-channel slice (one producing
      // wave, one scale) at a time
      f32x4 tot[NT];
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) tot[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c0 = 0; c0 < 8; c0 += 2) {               // two slices at a time: two independent accumulators interleaved
        f16x8 xh[2], xl[2];
        f32x4 a2[2][NT];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          xh[u] = *reinterpret_cast<const f16x8 *>(a2r + (16 * i2 + lr) * RS2 + (c0 + u) * 64 + g * 16);
          xl[u] = *reinterpret_cast<const f16x8 *>(a2r + A2_PLANE + (16 * i2 + lr) * RS2 + (c0 + u) * 64 + g * 16);
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) a2[u][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if constexpr (EXIT) {
          f16x8 wl[2][NT];
#pragma unroll
          for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
              wl[u][tt] = *reinterpret_cast<const f16x8 *>(lds + OFF_WL + ((((NT * q2 + tt) * 8) + c0 + u) * 64 + lane) * 16);
#pragma unroll
          for (int pr = 0; pr < 3; ++pr)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
              for (int tt = 0; tt < NT; ++tt)
                a2[u][tt] = ymi_mfma16(pr == 0 ? wl[u][tt] : w1h[tt][c0 + u], pr == 1 ? xl[u] : xh[u], a2[u][tt]);
        } else {
#pragma unroll
          for (int pr = 0; pr < 3; ++pr)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
              for (int tt = 0; tt < NT; ++tt)
                a2[u][tt] = ymi_mfma16(pr == 0 ? w1l[tt][c0 + u] : w1h[tt][c0 + u], pr == 1 ? xl[u] : xh[u], a2[u][tt]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const float isc = scr[i2 * NW + c0 + u];
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) tot[tt] += a2[u][tt] * isc;
        }
      }
      // P5: epilogue 2
      const int tp = tile - grid, m = tp * PX + 16 * i2 + lr;
      const bool ok = tp >= 0 && m < p.M;
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        if constexpr (EXIT) {
          sc1 = *reinterpret_cast<const f32x4 *>(lds + OFF_EP2 + ((wave * 2 + tt) * 4 + g) * 32);
          bi1 = *reinterpret_cast<const f32x4 *>(lds + OFF_EP2 + ((wave * 2 + tt) * 4 + g) * 32 + 16);
        }
        f32x4 v = tot[tt] * sc1 + bi1;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], slope_b * v[e]);
        am_z = fmaxf(am_z, ok ? ymi_absmax4(v) : 0.f);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), zrs,
                                               ok ? (unsigned)(m * p.ldz + 16 * NT * q2 + 16 * tt + 4 * g) * 4u : OOB, 0, 0);
      }
    }
    // P2 (tile k): GEMM 1 — both 16-pixel halves x this wave's two 16-channel tiles
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      f16x8 xh[2], xl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        xh[i] = *reinterpret_cast<const f16x8 *>(a1 + (16 * i + lr) * RS1 + c * 64 + g * 16);
        xl[i] = *reinterpret_cast<const f16x8 *>(a1 + A1_PLANE + (16 * i + lr) * RS1 + c * 64 + g * 16);
      }
#pragma unroll
      for (int pr = 0; pr < 3; ++pr)                    // (product-major: consecutive MFMAs belong to different accumulators)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = ymi_mfma16(pr == 0 ? w3l[j][c] : w3h[j][c], pr == 1 ? xl[i] : xh[i], acc[i][j]);
    }
    // P3 (tile k): epilogue 1 + this wave's 16 x 32 slices of y -> planes (one power-of-two scale per slice)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = tile * PX + 16 * i + lr;
      const bool ok = m < p.M;
      bool keep = ok;
      if constexpr (EXIT) {                             // y only where the stride-2 reader looks (no branch: the OOB offset again)
        const unsigned r = (unsigned)(((unsigned long long)(unsigned)m * p.mag_w) >> 32);          // m / W = b H + h
        const unsigned w = (unsigned)m - r * (unsigned)p.W;
        const unsigned h = r - (unsigned)(((unsigned long long)r * p.mag_h) >> 32) * (unsigned)p.H;
        keep = ok && (p.y_stride == 1 || ((h | w) & 1u) == 0);
      }
      const unsigned yoff = keep ? (unsigned)(m * p.ldy + 32 * wave + 4 * g) * 4u : OOB;
      // ENTRY: the shortcut's GEMM on this half of the x0 tile, same shape and product order as GEMM 1 (taken half by half, next to
      // the epilogue that consumes it: eight accumulator registers live instead of sixteen, which is what keeps the kernel out of scratch)
      f32x4 accd[2];
      if constexpr (ENTRY) {
#pragma unroll
        for (int j = 0; j < 2; ++j) accd[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          f16x8 wdl[2];
#pragma unroll
          for (int j = 0; j < 2; ++j) wdl[j] = *reinterpret_cast<const f16x8 *>(lds + OFF_WDL + (((wave * 2 + j) * 2 + c) * 64 + lane) * 16);
          const f16x8 xh = *reinterpret_cast<const f16x8 *>(a0 + (16 * i + lr) * RS1 + c * 64 + g * 16);
          const f16x8 xl = *reinterpret_cast<const f16x8 *>(a0 + A1_PLANE + (16 * i + lr) * RS1 + c * 64 + g * 16);
#pragma unroll
          for (int pr = 0; pr < 3; ++pr)
#pragma unroll
            for (int j = 0; j < 2; ++j)
              accd[j] = ymi_mfma16(pr == 0 ? wdl[j] : wdh[j][c], pr == 1 ? xl : xh, accd[j]);
        }
      }
      float tm = 0.f;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const f32x4 sc3 = *reinterpret_cast<const f32x4 *>(lds + OFF_EP + ((wave * 2 + j) * 4 + g) * 32);
        const f32x4 bi3 = *reinterpret_cast<const f32x4 *>(lds + OFF_EP + ((wave * 2 + j) * 4 + g) * 32 + 16);
        f32x4 v;
        if constexpr (ENTRY) {
          const f32x4 scd = *reinterpret_cast<const f32x4 *>(lds + OFF_EPD + ((wave * 2 + j) * 4 + g) * 32);
          const f32x4 bid = *reinterpret_cast<const f32x4 *>(lds + OFF_EPD + ((wave * 2 + j) * 4 + g) * 32 + 16);
          const f32x4 r = accd[j] * scd + bid;
          v = acc[i][j] * sc3 + bi3 + r;
        } else {
          v = acc[i][j] * sc3 + bi3 + rv[i][j];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], slope_a * v[e]);
        if (!ok) v = f32x4{0.f, 0.f, 0.f, 0.f};
        acc[i][j] = v;
        tm = fmaxf(tm, ymi_absmax4(v));
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), yrs, yoff + 64u * j, 0, 0);
      }
      am_y = fmaxf(am_y, tm);
      if (two) {
        const unsigned tmb = ymi_wave_umax63(__builtin_bit_cast(unsigned, tm));
        float sT, invT;
        ymi_h2_scale(__builtin_bit_cast(float, (unsigned)__builtin_amdgcn_readlane((int)tmb, 63)), sT, invT);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f32x4 v = acc[i][j] * sT;
          f16x4 h4, l4;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const _Float16 h = (_Float16)v[e];
            h4[e] = h;
            l4[e] = (_Float16)(v[e] - (float)h);
          }
          char *dst = a2w + (16 * i + lr) * RS2 + (32 * wave + 16 * j + 4 * g) * 2;
          *reinterpret_cast<f16x4 *>(dst) = h4;
          *reinterpret_cast<f16x4 *>(dst + A2_PLANE) = l4;
        }
        if (lane == 0) scw[i * NW + wave] = invT;
      }
    }
  };
  int tile = blockIdx.x;
  f32x4 ra[2][2], rb[2][2];
  xv = load_x(tile);
  if constexpr (ENTRY) x0v = load_x0(tile);
  else load_res(tile, ra);
  for (; tile < ntiles + (two ? grid : 0); tile += 2 * grid) {      // (+ one iteration for the last tile's second layer)
    iteration(tile, std::integral_constant<int, 0>{}, ra, rb);
    iteration(tile + grid, std::integral_constant<int, 1>{}, rb, ra);
  }
  if (p.y_amax) ymi_amax_finish(apre_y, am_y);
  if (two && p.z_amax) ymi_amax_finish(apre_z, am_z);
#endif
}

}  // namespace

// y = act_a(scale_a * (W_a x) + bias_a + res),  z = act_b(scale_b * (W_b y) + bias_b): two chained 1x1 convolutions, 64 -> 256 -> 64
// (include/yolact_amd.h, ymi_chain_desc).  Profiling: record kind 13 = the launch with conv A's algorithmic FLOPs, then — when z
// is computed — a kind-12 record (no duration of its own) carrying conv B's.  The ENTRY form (x0 != NULL) puts a kind-12 record
// with the shortcut's FLOPs between the two.
int ymi_internal_chain2(const ymi_chain_desc *d, hipStream_t s);    // csrc/chain2.hip: 128 / 256 planes, filters streamed through LDS

extern "C" int ymi_pointwise_chain_f32(const ymi_chain_desc *d, void *stream) {
  if (!d) return YMI_ENULL;
  if (!d->x || !d->w_a_h2 || !d->scale_a_h2 || !d->y || !d->x_amax) return YMI_ENULL;
  if (d->z && (!d->w_b_h2 || !d->scale_b_h2)) return YMI_ENULL;
  const bool wide = d->k_a == 128 || d->k_a == 256;
  if (d->M <= 0 || (!wide && (d->k_a != K1 || d->n_a != N1 || (d->z && d->n_b != 64)))) return YMI_EARG;
  if (wide && (d->n_a != 4 * d->k_a || (d->z && d->n_b != d->k_a))) return YMI_EARG;
  if (d->act_a < 0 || d->act_a > YMI_ACT_LEAKY01 || d->act_b < 0 || d->act_b > YMI_ACT_LEAKY01) return YMI_EARG;
  if (d->ldx < d->k_a || d->ldy < d->n_a || (d->z && d->ldz < d->n_b) || (d->res && d->res_ld < d->n_a)) return YMI_ESHAPE;
  if ((d->ldx | d->ldy | d->ldz | d->res_ld) & 3) return YMI_ESHAPE;
  if ((((uintptr_t)d->x) | ((uintptr_t)d->y) | ((uintptr_t)d->z) | ((uintptr_t)d->res) | ((uintptr_t)d->w_a_h2) | ((uintptr_t)d->w_b_h2)) & 15)
    return YMI_ESHAPE;
  if (d->M * (int64_t)(d->ldy > d->res_ld ? d->ldy : d->res_ld) >= (1LL << 29) || d->M * (int64_t)d->ldx >= (1LL << 29)) return YMI_ESHAPE;   // 32-bit buffer offsets
  const bool entry = d->x0 != nullptr;      // the ENTRY form: the residual is the projection shortcut of x0, computed in the launch
  if (entry) {
    if (wide || d->res || d->k_a != K1 || d->n_a != N1) return YMI_EARG;
    if (!d->w_d_h2 || !d->scale_d_h2 || !d->x0_amax) return YMI_ENULL;
    if (d->ldx0 < K1 || (d->ldx0 & 3) || ((((uintptr_t)d->x0) | ((uintptr_t)d->w_d_h2)) & 15)) return YMI_ESHAPE;
    if (d->M * (int64_t)d->ldx0 >= (1LL << 29) || d->cout_pad_d < N1) return YMI_ESHAPE;
  }
  if (wide) return ymi_internal_chain2(d, (hipStream_t)stream);
  if (d->cout_pad_a < N1 || (d->z && d->cout_pad_b < 64)) return YMI_ESHAPE;
  ChainParamsE p;                           // (sliced to ChainParams for the plain form: that kernel's argument layout is unchanged)
  p.x0 = d->x0; p.x0_amax = d->x0_amax; p.wd = d->w_d_h2; p.sd = d->scale_d_h2; p.bd = d->bias_d; p.ldx0 = d->ldx0;
  p.wd_plane = (unsigned)((long)d->cout_pad_d * K1 * 2);
  p.x = d->x; p.res = d->res; p.x_amax = d->x_amax; p.wa = d->w_a_h2; p.wb = d->w_b_h2;
  p.sa = d->scale_a_h2; p.ba = d->bias_a; p.sb = d->scale_b_h2; p.bb = d->bias_b;
  p.y = d->y; p.z = d->z; p.y_amax = d->y_amax; p.z_amax = d->z_amax;
  p.M = (int)d->M; p.ldx = d->ldx; p.res_ld = d->res_ld; p.ldy = d->ldy; p.ldz = d->ldz; p.act_a = d->act_a; p.act_b = d->act_b;
  p.wa_plane = (unsigned)((long)d->cout_pad_a * K1 * 2); p.wb_plane = (unsigned)((long)d->cout_pad_b * N1 * 2);
  hipStream_t s = (hipStream_t)stream;
  const int pr = ymi_internal_prof_begin(2.0 * (double)d->M * K1 * N1, YMI_TILE_H2 | YMI_TILE_64x64, 13, s);
  int dev = 0, cus = 256;
  hipGetDevice(&dev);
  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const long ntiles = (d->M + PX - 1) / PX;
  const dim3 grid((unsigned)(ntiles < cus ? ntiles : cus));
  if (entry) hipLaunchKernelGGL((chain_h2_k<64, true>), grid, dim3(64 * NW), 0, s, p);
  else hipLaunchKernelGGL(chain_h2_k<64>, grid, dim3(64 * NW), 0, s, static_cast<const ChainParams &>(p));
  const int rc = ymi_launch_status();
  ymi_internal_prof_end(pr, s);
  if (rc == YMI_OK && entry) {              // the shortcut's FLOPs: a kind-12 record of its own, between conv3's and conv1's
    const int pd = ymi_internal_prof_begin(2.0 * (double)d->M * K1 * N1, YMI_TILE_H2 | YMI_TILE_64x64, 12, s);
    ymi_internal_prof_end(pd, s);
  }
  if (rc == YMI_OK && d->z) {
    const int p2 = ymi_internal_prof_begin(2.0 * (double)d->M * N1 * 64, YMI_TILE_H2 | YMI_TILE_64x64, 12, s);
    ymi_internal_prof_end(p2, s);
  }
  return rc;
}

// The stage exit (include/yolact_amd.h, ymi_stage_exit_desc): y = act_a(scale_a * (W_a x) + bias_a + res) of layer0.2.conv3, stored
// only where the stride-2 shortcut of the next stage reads it, and z = act_b(scale_b * (W_b y) + bias_b) of layer1.0.conv1
// (256 -> 128) from the y tile in LDS.  Profiling records as the chain's: kind 13 (conv3's FLOPs), then kind 12 (conv1's).
extern "C" int ymi_stage_exit_chain_f32(const ymi_stage_exit_desc *e, void *stream) {
  if (!e) return YMI_ENULL;
  const ymi_chain_desc *d = &e->chain;
  if (!d->x || !d->w_a_h2 || !d->scale_a_h2 || !d->y || !d->x_amax || !d->z || !d->w_b_h2 || !d->scale_b_h2) return YMI_ENULL;
  if (d->k_a != K1 || d->n_a != N1 || d->n_b != 128 || (e->y_stride != 1 && e->y_stride != 2)) return YMI_EARG;
  if (d->x0) return YMI_EARG;               // the entry form belongs to the 64-wide pair
  if (d->M <= 0 || e->B <= 0 || e->H <= 0 || e->W <= 0 || d->M != (int64_t)e->B * e->H * e->W) return YMI_EARG;
  if (d->act_a < 0 || d->act_a > YMI_ACT_LEAKY01 || d->act_b < 0 || d->act_b > YMI_ACT_LEAKY01) return YMI_EARG;
  if (d->ldx < K1 || d->ldy < N1 || d->ldz < 128 || (d->res && d->res_ld < N1)) return YMI_ESHAPE;
  if ((d->ldx | d->ldy | d->ldz | d->res_ld) & 3) return YMI_ESHAPE;
  if ((((uintptr_t)d->x) | ((uintptr_t)d->y) | ((uintptr_t)d->z) | ((uintptr_t)d->res) | ((uintptr_t)d->w_a_h2) | ((uintptr_t)d->w_b_h2)) & 15)
    return YMI_ESHAPE;
  const int64_t ldmax = d->ldy > d->res_ld ? (d->ldy > d->ldz ? d->ldy : d->ldz) : (d->res_ld > d->ldz ? d->res_ld : d->ldz);
  if (d->M * ldmax >= (1LL << 29) || d->M * (int64_t)d->ldx >= (1LL << 29)) return YMI_ESHAPE;    // 32-bit buffer offsets
  if (d->cout_pad_a < N1 || d->cout_pad_b < 128) return YMI_ESHAPE;
  // the kernel decodes (h, w) of row m by multiplication with ceil(2^32 / W) and ceil(2^32 / H): exact for every m < M and every
  // m / W < B * H only while M * W < 2^32 and B * H * H < 2^32 (M alone bounds neither: a 10 x 100 000 map has M = 10^6)
  if (d->M * (int64_t)(e->H > e->W ? e->H : e->W) >= (1LL << 32)) return YMI_ESHAPE;
  ChainParamsX p;
  p.x = d->x; p.res = d->res; p.x_amax = d->x_amax; p.wa = d->w_a_h2; p.wb = d->w_b_h2;
  p.sa = d->scale_a_h2; p.ba = d->bias_a; p.sb = d->scale_b_h2; p.bb = d->bias_b;
  p.y = d->y; p.z = d->z; p.y_amax = d->y_amax; p.z_amax = d->z_amax;
  p.M = (int)d->M; p.ldx = d->ldx; p.res_ld = d->res_ld; p.ldy = d->ldy; p.ldz = d->ldz; p.act_a = d->act_a; p.act_b = d->act_b;
  p.wa_plane = (unsigned)((long)d->cout_pad_a * K1 * 2); p.wb_plane = (unsigned)((long)d->cout_pad_b * N1 * 2);
  p.H = e->H; p.W = e->W; p.y_stride = e->y_stride;
  p.mag_w = ((1ULL << 32) + (unsigned)e->W - 1) / (unsigned)e->W;
  p.mag_h = ((1ULL << 32) + (unsigned)e->H - 1) / (unsigned)e->H;
  hipStream_t s = (hipStream_t)stream;
  const int pr = ymi_internal_prof_begin(2.0 * (double)d->M * K1 * N1, YMI_TILE_H2 | YMI_TILE_64x64, 13, s);
  int dev = 0, cus = 256;
  hipGetDevice(&dev);
  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const long ntiles = (d->M + PX - 1) / PX;
  hipLaunchKernelGGL(chain_h2_k<128>, dim3((unsigned)(ntiles < cus ? ntiles : cus)), dim3(64 * NW), 0, s, p);
  const int rc = ymi_launch_status();
  ymi_internal_prof_end(pr, s);
  if (rc == YMI_OK) {
    const int p2 = ymi_internal_prof_begin(2.0 * (double)d->M * N1 * 128, YMI_TILE_H2 | YMI_TILE_64x64, 12, s);
    ymi_internal_prof_end(p2, s);
  }
  return rc;
}
