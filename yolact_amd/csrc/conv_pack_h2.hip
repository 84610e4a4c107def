// The filters of a training step as the fp16x2 tiles read them, packed on the device from the parameters' current storage.
//
//   ymi_conv_pack_h2_f32   w[i] [cout[i], Cin, k, k] (fp32, torch layout, i < n <= 3, output channels concatenated) ->
//                          planes int16 [2][RowsPad][Kp], winv fp32 [RowsPad] and, optionally, w32 fp32 [RowsPad][Kp].
//     mode 0 (forward)        row = output channel, Kp = k k Cin, column (ky k + kx) Cin + c          (train_ops._pack_forward)
//     mode 1 (data gradient)  row = input channel,  Kp = k k ld,  column (ky' k + kx') ld + co holds w[co, row, k-1-ky', k-1-kx'],
//                             columns co >= sum cout zero                                              (train_ops._pack_dgrad)
//
// Inference builds these planes on the host once per checkpoint (engine.split2_planes_f16); in training the parameters change every
// step.  Per row: s = ymi_h2_scale(max |w|) (csrc/common.h: the rule of the activations), plane 0 = fp16(w s), plane 1 =
// fp16(w s - plane 0), both by round to nearest even (gemm_h2.h split8h's arithmetic), winv = 1 / s.  The maximum is taken over the
// bit patterns of |w|, so a NaN anywhere in the row makes the maximum a NaN: a maximum of 0, Inf or NaN gives s = 1, the helper's rule.
// Rows [Rows, RowsPad) are zero with winv = 1.
//
// No atomics, no workspace: a block owns whole rows and makes two passes over their source, the maximum first, the split second
// (the second reads what the first left in L2).  Both layouts are transposes of the source, so both passes read it in contiguous
// runs, 4 bytes per lane (the parameters' storage is only 4-byte aligned), and turn it through LDS:
//   mode 0  one row per block of 256 threads.  The row's source is Cin k k contiguous floats, index c k k + t.  The split pass stages
//           256 channels at a time and each thread writes 4 consecutive channels of one tap: 8-byte plane stores, 128 bytes per 16
//           lanes.  The LDS reads are 36 floats apart between lanes (4-way on 32 banks): far above what the stores sustain.
//   mode 1  8 input channels and 128 output channels per block (576 threads at 3x3, 512 at 1x1).  For one output channel the block's
//           source is a run of 8 k k contiguous floats (288 bytes at 3x3, 32 at 1x1); a thread owns one element of the run, so
//           the first pass, over ALL output channels, is coalesced loads into one register maximum per thread.  The second
//           pass stages the block's 128 output channels as [128][8 k k + 1] and writes 4 consecutive output channels of one
//           (row, tap) per thread.
#include "loss_common.h"
#include "../../include/yolact_amd.h"

namespace {

struct PackParams {
  const float *w[3];
  unsigned short *planes;
  float *winv, *w32;
  int cout[3];
  int n, Cin, ld, ctot, rows, rows_pad, Kp;
};

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned abs_bits(float v) { return __builtin_bit_cast(unsigned, v) & 0x7fffffffu; }

// four values -> 4 consecutive elements of the two planes (and of w32) at element offset `at` (a multiple of 4)
__device__ __forceinline__ void store4(const PackParams &p, size_t at, const f32x4 v, float s) {
  u16x4 h, l;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float t = v[e] * s;
    const _Float16 hh = (_Float16)t;
    const _Float16 ll = (_Float16)(t - (float)hh);
    h[e] = __builtin_bit_cast(unsigned short, hh);
    l[e] = __builtin_bit_cast(unsigned short, ll);
  }
  *reinterpret_cast<u16x4 *>(p.planes + at) = h;
  *reinterpret_cast<u16x4 *>(p.planes + (size_t)p.rows_pad * p.Kp + at) = l;
  if (p.w32) *reinterpret_cast<f32x4 *>(p.w32 + at) = v;
}

// rows [row0, row0 + nrows) past the last real one: zero planes, winv = 1
__device__ __forceinline__ void zero_rows(const PackParams &p, int row0, int nrows, int nthr) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const size_t base = (size_t)row0 * p.Kp;
  for (int i = threadIdx.x; i < nrows * (p.Kp / 4); i += nthr) store4(p, base + 4 * (size_t)i, z, 1.f);
  if ((int)threadIdx.x < nrows) p.winv[row0 + threadIdx.x] = 1.f;
}

// concatenated output channel -> (its tensor, the channel within it)
__device__ __forceinline__ const float *locate(const PackParams &p, int co, int &local) {
  int i = 0;
  while (i < p.n - 1 && co >= p.cout[i]) { co -= p.cout[i]; ++i; }
  local = co;
  return p.w[i];
}

constexpr int FWD_THREADS = 256, FWD_CC = 256;        // mode 0: channels staged at a time

template <int KK>
__global__ __launch_bounds__(FWD_THREADS) void pack_fwd_k(const PackParams p) {
  __shared__ float buf[FWD_CC * KK];
  __shared__ unsigned red[FWD_THREADS / 64];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (r >= p.rows) { zero_rows(p, r, 1, FWD_THREADS); return; }
  int local;
  const float *src = locate(p, r, local);
  src += (size_t)local * p.Cin * KK;
  // pass 1: the row's maximum
  unsigned m = 0;
  for (int j = tid; j < p.Kp; j += FWD_THREADS) { const unsigned b = abs_bits(src[j]); m = b > m ? b : m; }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { const unsigned o = (unsigned)__shfl_xor((int)m, off, 64); m = o > m ? o : m; }
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < FWD_THREADS / 64; ++i) m = red[i] > m ? red[i] : m;
  float s, inv;
  ymi_h2_scale(__builtin_bit_cast(float, m), s, inv);
  if (tid == 0) p.winv[r] = inv;
  // pass 2: FWD_CC channels at a time through LDS
  for (int c0 = 0; c0 < p.Cin; c0 += FWD_CC) {
    const int nc = p.Cin - c0 < FWD_CC ? p.Cin - c0 : FWD_CC;          // a multiple of 32
    __syncthreads();
    for (int j = tid; j < nc * KK; j += FWD_THREADS) buf[j] = src[(size_t)c0 * KK + j];
    __syncthreads();
    const int q = nc / 4;
    for (int it = tid; it < q * KK; it += FWD_THREADS) {
      const int t = it / q, c = 4 * (it - t * q);
      const f32x4 v = {buf[c * KK + t], buf[(c + 1) * KK + t], buf[(c + 2) * KK + t], buf[(c + 3) * KK + t]};
      store4(p, (size_t)r * p.Kp + (size_t)t * p.Cin + c0 + c, v, s);
    }
  }
}

constexpr int DG_RB = 8, DG_COT = 128;              // mode 1: rows per block, output channels per block

// the source of concatenated output channel co (co < ctot), at its input channel 0
template <int KK>
__device__ __forceinline__ const float *filter_of(const PackParams &p, int co) {
  int local;
  const float *w = locate(p, co, local);
  return w + (size_t)local * p.Cin * KK;
}

// Block (x, y): input channels [8 x, 8 x + 8), output channels [128 y, 128 y + 128).  NT = PAR * R threads, R = 8 k k the length of
// the block's contiguous run in one filter: thread (c, j) reads element j of the runs of the output channels c, c + PAR, ..; all its
// elements belong to one row, so the first pass keeps one running maximum per thread and needs LDS only for the last step.  Every
// block of a row group repeats that pass over ALL output channels (reads that hit L2), so that no block waits for another.
template <int KK, int NT>
__global__ __launch_bounds__(NT) void pack_dgrad_k(const PackParams p) {
  constexpr int R = DG_RB * KK, LD = R + 1, PAR = NT / R;
  static_assert(NT == PAR * R, "one thread per (output channel in flight, element of the run)");
  __shared__ float tile[DG_COT * LD];
  __shared__ unsigned red[NT];
  __shared__ float srow[DG_RB];
  const int ci0 = blockIdx.x * DG_RB, co0 = blockIdx.y * DG_COT, tid = threadIdx.x;
  if (ci0 >= p.rows) {                                  // (Cin % 32 == 0: a block is all real or all padding)
    if (blockIdx.y == 0) zero_rows(p, ci0, DG_RB, NT);
    return;
  }
  const int j = tid % R, cl = tid / R;
  const size_t off = (size_t)ci0 * KK + j;
  // pass 1: the maxima of the block's rows over every output channel
  unsigned m = 0;
#pragma unroll 4
  for (int co = cl; co < p.ctot; co += PAR) { const unsigned b = abs_bits(filter_of<KK>(p, co)[off]); m = b > m ? b : m; }
  red[tid] = m;
  __syncthreads();
  if (tid < DG_RB) {
    unsigned mm = 0;
    for (int c = 0; c < PAR; ++c)
#pragma unroll
      for (int t = 0; t < KK; ++t) { const unsigned b = red[c * R + tid * KK + t]; mm = b > mm ? b : mm; }
    float s, inv;
    ymi_h2_scale(__builtin_bit_cast(float, mm), s, inv);
    srow[tid] = s;
    if (blockIdx.y == 0) p.winv[ci0 + tid] = inv;
  }
  // pass 2: the block's own output channels through LDS; the columns [ctot, ld) read zeros
#pragma unroll 4
  for (int co = cl; co < DG_COT; co += PAR) tile[co * LD + j] = co0 + co < p.ctot ? filter_of<KK>(p, co0 + co)[off] : 0.f;
  __syncthreads();                                      // (publishes srow too)
  for (int it = tid; it < DG_RB * KK * (DG_COT / 4); it += NT) {
    const int co = 4 * (it & (DG_COT / 4 - 1)), rt = it / (DG_COT / 4);
    const int row = rt / KK, t = rt - row * KK;
    if (co0 + co < p.ld) {                              // ld % 32 == 0: the four columns exist together
      const int at = row * KK + (KK - 1 - t);           // both taps flipped: tap index k k - 1 - t
      const f32x4 v = {tile[co * LD + at], tile[(co + 1) * LD + at], tile[(co + 2) * LD + at], tile[(co + 3) * LD + at]};
      store4(p, (size_t)(ci0 + row) * p.Kp + (size_t)t * p.ld + co0 + co, v, srow[row]);
    }
  }
}

int validate_pack(const ymi_conv_pack_desc *d, PackParams &p) {
  if (!d) return YMI_ENULL;
  if (d->n < 1 || d->n > 3) return YMI_EARG;
  if ((d->k != 1 && d->k != 3) || (d->mode != 0 && d->mode != 1) || d->Cin < 1) return YMI_EARG;
  long ctot = 0;
  for (int i = 0; i < d->n; ++i) {
    if (d->cout[i] < 1) return YMI_EARG;
    ctot += d->cout[i];
  }
  if (!d->planes || !d->winv) return YMI_ENULL;
  for (int i = 0; i < d->n; ++i) if (!d->w[i]) return YMI_ENULL;
  if (d->Cin % 32 != 0) return YMI_ESHAPE;
  if (d->mode == 1 && (d->ld % 32 != 0 || d->ld < ctot)) return YMI_ESHAPE;
  if (((uintptr_t)d->planes | (uintptr_t)d->winv | (uintptr_t)d->w32) & 15) return YMI_ESHAPE;
  const long rows = d->mode == 0 ? ctot : d->Cin, rows_pad = (rows + 127) / 128 * 128;
  const long Kp = (long)d->k * d->k * (d->mode == 0 ? d->Cin : d->ld);
  if (rows_pad * Kp >= (1L << 29)) return YMI_ESHAPE;
  for (int i = 0; i < 3; ++i) { p.w[i] = i < d->n ? d->w[i] : nullptr; p.cout[i] = i < d->n ? d->cout[i] : 0; }
  p.planes = (unsigned short *)d->planes; p.winv = d->winv; p.w32 = d->w32;
  p.n = d->n; p.Cin = d->Cin; p.ld = d->mode == 1 ? d->ld : 0; p.ctot = (int)ctot;
  p.rows = (int)rows; p.rows_pad = (int)rows_pad; p.Kp = (int)Kp;
  return YMI_OK;
}

}  // namespace

extern "C" int ymi_conv_pack_h2_f32(const ymi_conv_pack_desc *d, void *stream) {
  PackParams p;
  const int rc = validate_pack(d, p);
  if (rc) return rc;
  if (d->mode == 0) {
    const dim3 grid((unsigned)p.rows_pad);
    return d->k == 3 ? ymi_launch(pack_fwd_k<9>, grid, dim3(FWD_THREADS), 0, stream, p)
                     : ymi_launch(pack_fwd_k<1>, grid, dim3(FWD_THREADS), 0, stream, p);
  }
  const dim3 grid((unsigned)(p.rows_pad / DG_RB), (unsigned)((p.ld + DG_COT - 1) / DG_COT));
  return d->k == 3 ? ymi_launch(pack_dgrad_k<9, 8 * DG_RB * 9>, grid, dim3(8 * DG_RB * 9), 0, stream, p)
                   : ymi_launch(pack_dgrad_k<1, 64 * DG_RB>, grid, dim3(64 * DG_RB), 0, stream, p);
}
