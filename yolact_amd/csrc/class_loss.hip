// The class term 'C' of MultiBoxLoss with online hard example mining (layers/modules/multibox_loss.py:242-296 ohem_conf_loss, for
// ohem_use_most_confident = use_class_balanced_conf = False), loss and gradient for a whole batch.  The reference materialises a
// log_sum_exp over conf_data, sorts [B,P] twice for ranks, builds two [B,P,C] masks, gathers through them and lets autograd
// scatter back; here:
//
// cl_keys_k    grid (row tiles, images).  The tile's rows are one contiguous span of conf (a row of 81 floats is never 16-byte
//              aligned, the span is loaded with 16-byte loads where they fit); in LDS a row has an ODD stride, so that one thread
//              per row reduces its row without bank conflicts.  Writes lse = logsumexp(row) (the row's own maximum subtracted),
//              the mining key lse - row[0] (0 for positives and neutrals) and the tile's count of positives.
// cl_select_k  one workgroup per image: n = min(negpos_ratio * num_pos, P - 1), then an exact radix select of the n-th largest key
//              (keys are non-negative floats, their bit patterns order as unsigned integers; four 8-bit digits, a 256-bin LDS
//              histogram of integer atomics, whose result does not depend on their order).  Keys equal to the threshold are taken
//              in prior order (the lowest index wins) by an index-ordered prefix count.  neg = marked and conf_t == 0.
// cl_grad_k    grid (row tiles, images): the loss term lse - row[conf_t] of every row of pos | neg (for a negative the bits of its
//              key) summed per tile, and d_conf = alpha (exp(x - lse) - onehot) on those rows, +0.0f on every other row.
// cl_sum_k     one block: the loss from the per-tile partials in a fixed order.
//
// No floating-point atomics, no cooperative grid, no waiting between blocks: the same inputs give the same bits.  A label is
// compared with its range before it indexes anything; one outside -1 .. C-1 makes the loss NaN.
// Bound by memory traffic: launch 1 reads conf once, launch 3 writes d_conf once and re-reads only the selected rows.
#include "loss_common.h"
#include "../../include/yolact_amd.h"

#pragma clang fp contract(off)

namespace {

constexpr int CT = 128;          // threads of cl_keys_k / cl_grad_k = the most rows of a tile
constexpr int LDS_F = 10752;     // floats of the row tile in LDS: 128 rows of stride 83
constexpr int ST = 1024;         // threads of cl_select_k

struct ClParams {
  const float *conf;
  const int32_t *conf_t;
  float *loss, *d_conf;
  uint8_t *neg;
  int32_t *num_neg;
  float *ws_key, *ws_lse;        // [B][P]
  int32_t *ws_cnt;               // [B][ntiles] positives of a tile
  float *ws_ls;                  // [B][ntiles] loss partial of a tile
  int B, P, C, Cs, R, ntiles, ratio;
  float alpha;
};

int stride_of(int C) { return C | 1; }                       // odd: thread t reads word t * Cs + j, all banks distinct
int rows_of(int C) { const int r = LDS_F / stride_of(C); return r < CT ? r : CT; }
int ntiles_of(int P, int C) { const int r = rows_of(C); return (P + r - 1) / r; }

__global__ __launch_bounds__(CT) void cl_keys_k(const ClParams p) {
  __shared__ float tile[LDS_F];
  __shared__ int cw[CT / 64];
  const int t = threadIdx.x, b = blockIdx.y;
  const int r0 = blockIdx.x * p.R;
  const int nr = p.P - r0 < p.R ? p.P - r0 : p.R;
  const long e0 = ((long)b * p.P + r0) * p.C, e1 = e0 + (long)nr * p.C;       // the span [e0, e1) of conf
  const bool linear = p.Cs == p.C;
  for (long v = (e0 >> 2) + t; v * 4 < e1; v += CT) {
    const long a = v * 4;
    float x[4];
    if (a >= e0 && a + 4 <= e1) {
      const f32x4 q = *reinterpret_cast<const f32x4 *>(p.conf + a);
      x[0] = q[0]; x[1] = q[1]; x[2] = q[2]; x[3] = q[3];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = (a + k >= e0 && a + k < e1) ? p.conf[a + k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long e = a + k;
      if (e < e0 || e >= e1) continue;
      const int rel = (int)(e - e0);
      const int at = linear ? rel : (rel / p.C) * p.Cs + rel % p.C;
      tile[at] = x[k];
    }
  }
  __syncthreads();
  bool positive = false;
  if (t < nr) {
    const float *row = tile + t * p.Cs;
    float m = row[0];
    for (int j = 1; j < p.C; ++j) m = fmaxf(m, row[j]);
    float s = 0.f;
    for (int j = 0; j < p.C; ++j) s += expf(row[j] - m);
    const float lse = m + logf(s);
    float key = lse - row[0];
    if (!(key >= 0.f)) key = key != key ? ymi_qnan() : 0.f;   // a NaN row sorts first, as torch.sort puts it
    const size_t o = (size_t)b * p.P + r0 + t;
    const int ct = p.conf_t[o];
    positive = ct > 0;
    p.ws_lse[o] = lse;
    p.ws_key[o] = ct == 0 ? key : 0.f;                                        // :255-256
  }
  const int c = ymi_wave_count(positive);
  if ((t & 63) == 0) cw[t >> 6] = c;
  __syncthreads();
  if (t == 0) p.ws_cnt[(size_t)b * p.ntiles + blockIdx.x] = ymi_waves_count<CT / 64>(cw);
}

__global__ __launch_bounds__(ST) void cl_select_k(const ClParams p) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_k;
  __shared__ int wtake[ST / 64], wneg[ST / 64];
  __shared__ int s_base, s_nneg;
  const int t = threadIdx.x, b = blockIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned *key = reinterpret_cast<const unsigned *>(p.ws_key) + (size_t)b * p.P;
  const int32_t *ct = p.conf_t + (size_t)b * p.P;
  uint8_t *neg = p.neg + (size_t)b * p.P;

  // num_pos: the tile counts strided over the workgroup, a wave butterfly, the waves through LDS (integers: any order, one value)
  int c = 0;
  for (int tl = t; tl < p.ntiles; tl += ST) c += p.ws_cnt[(size_t)b * p.ntiles + tl];
  c = ymi_wave_sum(c);
  if (lane == 0) wtake[wave] = c;
  __syncthreads();
  long num_pos = 0;
  for (int w = 0; w < ST / 64; ++w) num_pos += wtake[w];
  __syncthreads();                                     // wtake is written again below
  long n = num_pos * p.ratio;
  if (n > p.P - 1) n = p.P - 1;                                                              // :260
  if (n <= 0) {                                                                              // uniform
    for (int i = t; i < p.P; i += ST) neg[i] = 0;
    if (t == 0) p.num_neg[b] = 0;
    return;
  }
  // the n-th largest key T: digit by digit from the top; k = how many keys are still to take among those that share the prefix
  if (t == 0) { s_prefix = 0u; s_k = (unsigned)n; }
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (t < 256) hist[t] = 0u;
    __syncthreads();
    const unsigned prefix = s_prefix, k = s_k;
    const unsigned himask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
    for (int i = t; i < p.P; i += ST) {
      const unsigned v = key[i];
      if ((v & himask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (t < 256) {
      unsigned above = 0u;
      for (int d = t + 1; d < 256; ++d) above += hist[d];
      const unsigned h = hist[t];
      if (above < k && k <= above + h) { s_prefix = prefix | ((unsigned)t << shift); s_k = k - above; }   // exactly one bin
    }
    __syncthreads();
  }
  const unsigned T = s_prefix;
  const int k = (int)s_k;                              // keys equal to T that are taken: the first k in prior order
  if (t == 0) { s_base = 0; s_nneg = 0; }
  __syncthreads();
  for (int i0 = 0; i0 < p.P; i0 += ST) {               // uniform trip count
    const int i = i0 + t;
    const bool ok = i < p.P;
    const unsigned v = ok ? key[i] : 0u;
    const bool eq = ok && v == T, gt = ok && v > T;
    const unsigned long long m = __ballot(eq);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wtake[wave] = __popcll(m);
    __syncthreads();
    int rank = s_base + before;
    for (int w = 0; w < wave; ++w) rank += wtake[w];
    const bool marked = gt || (eq && rank < k);
    const bool isneg = marked && ct[i < p.P ? i : 0] == 0;                      // :261-265
    if (ok) neg[i] = isneg ? 1 : 0;
    const int cn = __popcll(__ballot(isneg));
    if (lane == 0) wneg[wave] = cn;
    __syncthreads();
    if (t == 0) {
      int a = s_base, c = s_nneg;
      for (int w = 0; w < ST / 64; ++w) { a += wtake[w]; c += wneg[w]; }
      s_base = a; s_nneg = c;
    }
    __syncthreads();
  }
  if (t == 0) p.num_neg[b] = s_nneg;
}

__global__ __launch_bounds__(CT) void cl_grad_k(const ClParams p) {
  __shared__ float s_lse[CT];
  __shared__ int s_ct[CT];           // the label of a selected row; -1: the row is not selected; -2: selected, label out of range
  __shared__ float lw[CT / 64];
  const int t = threadIdx.x, b = blockIdx.y;
  const int r0 = blockIdx.x * p.R;
  const int nr = p.P - r0 < p.R ? p.P - r0 : p.R;
  float l = 0.f;
  if (t < nr) {
    const size_t o = (size_t)b * p.P + r0 + t;
    const int ct = p.conf_t[o];
    const float lse = p.ws_lse[o];
    int tag = -1;
    if (ct < -1 || ct >= p.C) { tag = -2; l = ymi_qnan(); }   // before it indexes
    else if (ct > 0 || (ct == 0 && p.neg[o])) { tag = ct; l = lse - p.conf[o * p.C + ct]; }
    s_lse[t] = lse; s_ct[t] = tag;
  }
  const float s = ymi_block_sum<CT / 64>(l, lw);
  if (t == 0) p.ws_ls[(size_t)b * p.ntiles + blockIdx.x] = s;
  if (!p.d_conf) return;                                                      // uniform

  const long e0 = ((long)b * p.P + r0) * p.C, e1 = e0 + (long)nr * p.C;
  for (long v = (e0 >> 2) + t; v * 4 < e1; v += CT) {
    const long a = v * 4;
    const long lo = a < e0 ? e0 : a, hi = a + 4 > e1 ? e1 : a + 4;
    int row = (int)((lo - e0) / p.C);
    int col = (int)((lo - e0) - (long)row * p.C);
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    for (long e = lo; e < hi; ++e) {
      const int tag = s_ct[row];
      if (tag >= 0) g[e - a] = p.alpha * (expf(p.conf[e] - s_lse[row]) - (col == tag ? 1.f : 0.f));
      else if (tag == -2) g[e - a] = ymi_qnan();
      if (++col == p.C) { col = 0; ++row; }
    }
    if (lo == a && hi == a + 4) {
      const f32x4 q = {g[0], g[1], g[2], g[3]};
      *reinterpret_cast<f32x4 *>(p.d_conf + a) = q;
    } else {
      for (long e = lo; e < hi; ++e) p.d_conf[e] = g[e - a];
    }
  }
}

// one block: loss = alpha * the B * ntiles partials, strided sums then a fixed tree
__global__ __launch_bounds__(256) void cl_sum_k(const ClParams p) {
  const float s = ymi_sum256(p.ws_ls, (long)p.B * p.ntiles);
  if (threadIdx.x == 0) p.loss[0] = s * p.alpha;
}

int validate_shape(const ymi_class_loss_desc *d) {
  if (!d) return YMI_ENULL;
  if (d->B < 1 || d->B > 65535 || d->P < 2 || d->C < 2 || d->C > 256 || d->negpos_ratio < 0) return YMI_EARG;
  if ((int64_t)d->B * d->P * d->C >= ((int64_t)1 << 31)) return YMI_ESHAPE;
  return YMI_OK;
}

// byte offsets of key, lse, cnt, ls; returns the total
int64_t layout(const ymi_class_loss_desc *d, int64_t (&off)[4]) {
  const int64_t BP = (int64_t)d->B * d->P, BT = (int64_t)d->B * ntiles_of(d->P, d->C);
  const int64_t sizes[4] = {BP, BP, BT, BT};
  return ymi_ws_layout(sizes, off);
}

}  // namespace

extern "C" int64_t ymi_class_loss_ws_bytes(const ymi_class_loss_desc *d) {
  const int rc = validate_shape(d);
  if (rc) return rc;
  int64_t off[4];
  return layout(d, off);
}

extern "C" int ymi_class_loss_f32(const ymi_class_loss_desc *d, void *stream) {
  const int rc = validate_shape(d);
  if (rc) return rc;
  if (!d->conf || !d->conf_t || !d->loss || !d->neg || !d->num_neg || !d->ws) return YMI_ENULL;
  if (((uintptr_t)d->conf | (uintptr_t)d->d_conf | (uintptr_t)d->ws) & 15) return YMI_ESHAPE;

  ClParams p = {};
  p.conf = d->conf; p.conf_t = d->conf_t; p.loss = d->loss; p.d_conf = d->d_conf; p.neg = d->neg; p.num_neg = d->num_neg;
  p.B = d->B; p.P = d->P; p.C = d->C; p.Cs = stride_of(d->C); p.R = rows_of(d->C); p.ntiles = ntiles_of(d->P, d->C);
  p.ratio = d->negpos_ratio; p.alpha = d->conf_alpha;
  int64_t off[4];
  layout(d, off);
  char *w = static_cast<char *>(d->ws);
  p.ws_key = (float *)(w + off[0]); p.ws_lse = (float *)(w + off[1]);
  p.ws_cnt = (int32_t *)(w + off[2]); p.ws_ls = (float *)(w + off[3]);

  int rl = ymi_launch(cl_keys_k, dim3(p.ntiles, d->B), dim3(CT), 0, stream, p);
  if (!rl) rl = ymi_launch(cl_select_k, dim3(d->B), dim3(ST), 0, stream, p);
  if (!rl) rl = ymi_launch(cl_grad_k, dim3(p.ntiles, d->B), dim3(CT), 0, stream, p);
  if (!rl) rl = ymi_launch(cl_sum_k, dim3(1), dim3(256), 0, stream, p);
  return rl;
}
