// MultiBoxLoss target assignment and the box loss 'B' for a whole batch (layers/box_utils.py:159-265 match / encode and the loop
// around it at layers/modules/multibox_loss.py:84-145, for use_prediction_matching = use_change_matching = use_yolo_regressors =
// False).  The reference builds an [n_gt, P] overlap matrix per image and runs a Python loop of n_gt iterations over it; here no
// overlap matrix exists and nothing returns to the host:
//
// match_best_k    grid (prior tiles, images), one thread = one prior.  The image's GT boxes pass through LDS in chunks of GC.  A
//                 thread keeps its prior's best (overlap, GT), and its best crowd ratio; per GT the tile reduces its best
//                 (overlap, lowest prior) into the workspace slot [tile][gt].
// match_force_k   one workgroup per image: the reference's greedy loop (box_utils.py:189-207).  Row state = each GT's (max, argmax)
//                 over the live columns, merged from the tile partials.  An iteration retires the row j with the largest max and
//                 its argmax column i (forced[i] = j); only the live rows whose argmax was i are recomputed, by re-evaluating
//                 that row's IoU against every prior with the whole workgroup (retired columns count -1, as in the reference).
// match_finish_k  grid (prior tiles, images): forced pairs, labels, thresholds, crowd rule, gt_box_t, encode, pos, and - with
//                 loc_data - the smooth-L1 partial of the tile and d_loc.
// match_sum_k     one block: num_pos per image and the loss from the per-tile partials, in a fixed order.
//
// Every IoU is evaluated by the one function iou() in the reference's operation order without FMA contraction and with IEEE
// division, so the three places that evaluate it agree to the bit with each other and with torch's CPU jaccard.  Every arg-max
// keeps the LOWEST index among equal values.  No atomics, no cooperative grid: the same inputs give the same bits.
// Nothing here is bound by arithmetic: launch 1 and 3 by their few hundred KB of traffic and the launch itself, launch 2 by the
// chain of n_gt dependent workgroup reductions.
#include "loss_common.h"
#include "../../include/yolact_amd.h"

#pragma clang fp contract(off)

namespace {

constexpr int TP = 256;      // priors per tile (one per thread) in match_best_k / match_finish_k
constexpr int GC = 64;       // GT boxes staged in LDS at once
constexpr int FT = 1024;     // threads of match_force_k
constexpr int RCAP = 256;    // rows whose state match_force_k keeps in LDS (more: in the workspace)

struct MtParams {
  const float *priors, *truth, *crowd, *loc_data;
  const int32_t *label, *gt_off, *crowd_off;
  const float *loc_t_in;       // box loss alone: the targets and positives are inputs
  const uint8_t *pos_in;
  float *loc_t, *gt_box_t, *d_loc, *loss;
  int32_t *conf_t, *idx_t, *num_pos;
  uint8_t *pos;
  float *ws_pv; int32_t *ws_pi;        // [ntiles][G]  best (overlap, prior) of a tile per GT
  float *ws_bto; int32_t *ws_bti;      // [B][P]       best (overlap, GT of the image) per prior
  float *ws_bco;                       // [B][P]       best crowd ratio per prior
  int32_t *ws_forced;                  // [B][P]       -1, or the GT the greedy loop forces on the prior
  float *ws_rmax; int32_t *ws_rarg;    // [G]          row state of images with more than RCAP GTs
  int32_t *ws_cnt; float *ws_ls;       // [B][ntiles]  positives / smooth-L1 sum of a tile
  int B, P, G, Gc, ntiles;
  float pos_thresh, neg_thresh, crowd_thresh, alpha;
};

struct Box { float x1, y1, x2, y2; };

__device__ __forceinline__ Box load_box(const float *p) {
  const f32x4 v = *reinterpret_cast<const f32x4 *>(p);
  return Box{v[0], v[1], v[2], v[3]};
}

// point_form (box_utils.py:16-17): centre -+ size / 2
__device__ __forceinline__ Box prior_box(const float *priors, int i) {
  const f32x4 v = *reinterpret_cast<const f32x4 *>(priors + (size_t)i * 4);
  return Box{v[0] - v[2] / 2.f, v[1] - v[3] / 2.f, v[0] + v[2] / 2.f, v[1] + v[3] / 2.f};
}

__device__ __forceinline__ float area(const Box &b) { return (b.x2 - b.x1) * (b.y2 - b.y1); }

// box_utils.py:47-51
__device__ __forceinline__ float inter(const Box &a, const Box &b) {
  float iw = fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1), ih = fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1);
  iw = iw < 0.f ? 0.f : iw; ih = ih < 0.f ? 0.f : ih;
  return iw * ih;
}

// box_utils.py:77-79: inter / (area_a + area_b - inter), a = the GT, b = the prior
__device__ __forceinline__ float iou(const Box &gt, float area_gt, const Box &pr, float area_pr) {
  const float in = inter(gt, pr);
  return __fdiv_rn(in, (area_gt + area_pr) - in);
}

// (v, i) <- the better of (v, i) and (ov, oi): the larger value, the lower index among equal values
__device__ __forceinline__ void take_better(float &v, int &i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__device__ __forceinline__ void wave_argmax(float &v, int &i) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float ov = __shfl_xor(v, d);
    const int oi = __shfl_xor(i, d);
    take_better(v, i, ov, oi);
  }
}

__global__ __launch_bounds__(TP) void match_best_k(const MtParams p) {
  __shared__ Box gts[GC];
  __shared__ float gar[GC];
  __shared__ float redv[4][GC];
  __shared__ int redi[4][GC];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int tile = blockIdx.x, b = blockIdx.y;
  const int pr = tile * TP + t;
  const bool ok = pr < p.P;
  const Box pb = prior_box(p.priors, ok ? pr : 0);
  const float pa = area(pb);
  int g0, n;
  ymi_image_range(p.gt_off, b, p.G, g0, n, p.P);

  float bto = -2.f;                                    // below every overlap: the first GT always replaces it
  int bti = 0;
  for (int c0 = 0; c0 < n; c0 += GC) {
    const int cnt = n - c0 < GC ? n - c0 : GC;
    __syncthreads();                                   // the previous chunk has been read
    if (t < cnt) {
      gts[t] = load_box(p.truth + (size_t)(g0 + c0 + t) * 4);
      gar[t] = area(gts[t]);
    }
    __syncthreads();
    for (int u = 0; u < cnt; ++u) {
      float v = ok ? iou(gts[u], gar[u], pb, pa) : -2.f;
      if (v > bto) { bto = v; bti = c0 + u; }          // overlaps.max(0): the lowest GT among equals
      int i = pr;
      wave_argmax(v, i);
      if (lane == 0) { redv[wave][u] = v; redi[wave][u] = i; }
    }
    __syncthreads();
    if (t < cnt) {
      float v = redv[0][t];
      int i = redi[0][t];
#pragma unroll
      for (int w = 1; w < 4; ++w) take_better(v, i, redv[w][t], redi[w][t]);
      const size_t slot = (size_t)tile * p.G + (g0 + c0 + t);
      p.ws_pv[slot] = v; p.ws_pi[slot] = i;
    }
  }
  if (!ok) return;
  const size_t o = (size_t)b * p.P + pr;
  p.ws_bto[o] = bto; p.ws_bti[o] = bti; p.ws_forced[o] = -1;
  if (p.Gc > 0) {
    // jaccard(decoded_priors, crowd_boxes, iscrowd=True).max(1): inter / area of the PRIOR (box_utils.py:79,218-220)
    int c0, nc;
    ymi_image_range(p.crowd_off, b, p.Gc, c0, nc);
    float bco = -1.f;
    for (int c = 0; c < nc; ++c) {
      const Box cb = load_box(p.crowd + (size_t)(c0 + c) * 4);
      const float v = __fdiv_rn(inter(pb, cb), pa);
      if (v > bco) bco = v;
    }
    p.ws_bco[o] = bco;
  }
}

// the workgroup's best (v, i); every thread returns it.  wv / wi: FT / 64 slots.
__device__ __forceinline__ void block_argmax(float &v, int &i, float *wv, int *wi) {
  wave_argmax(v, i);
  if ((threadIdx.x & 63) == 0) { wv[threadIdx.x >> 6] = v; wi[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = wv[0]; i = wi[0];
#pragma unroll
  for (int w = 1; w < FT / 64; ++w) take_better(v, i, wv[w], wi[w]);
  __syncthreads();                                     // wv / wi may be written again
}

__global__ __launch_bounds__(FT) void match_force_k(const MtParams p) {
  __shared__ float s_rmax[RCAP];
  __shared__ int s_rarg[RCAP];
  __shared__ float wv[FT / 64];
  __shared__ int wi[FT / 64];
  const int t = threadIdx.x, b = blockIdx.x;
  int g0, n;
  ymi_image_range(p.gt_off, b, p.G, g0, n, p.P);
  // row r: rmax = its largest overlap over the live columns (-1 once the row is retired), rarg = the lowest column that has it
  float *rmax = n <= RCAP ? s_rmax : p.ws_rmax + g0;
  int *rarg = n <= RCAP ? s_rarg : p.ws_rarg + g0;
  int32_t *forced = p.ws_forced + (size_t)b * p.P;

  for (int r = t; r < n; r += FT) {
    float v = -2.f;
    int i = 0;
    for (int tl = 0; tl < p.ntiles; ++tl) {            // tiles in prior order: a strict > keeps the lowest prior
      const size_t slot = (size_t)tl * p.G + (g0 + r);
      const float ov = p.ws_pv[slot];
      if (ov > v) { v = ov; i = p.ws_pi[slot]; }
    }
    rmax[r] = v; rarg[r] = i;
  }
  __syncthreads();

  for (int it = 0; it < n; ++it) {
    // j = best_prior_overlap.max(0)[1]: a live row has a max >= 0 (it < n <= P leaves it a live column), a retired one -1
    float v = -2.f;                                    // a thread without rows: below every row, retired ones included
    int j = 0;
    for (int r = t; r < n; r += FT) take_better(v, j, rmax[r], r);
    block_argmax(v, j, wv, wi);
    const int i = rarg[j];                             // in range: written from prior indices below P
    __syncthreads();                                   // everybody has read row j
    if (t == 0) { forced[i] = j; rmax[j] = -1.f; }
    __syncthreads();
    for (int r = 0; r < n; ++r) {
      // uniform: row r is rewritten only after the barriers of its own block_argmax
      if (rarg[r] != i || rmax[r] < 0.f) continue;
      const Box gb = load_box(p.truth + (size_t)(g0 + r) * 4);
      const float ga = area(gb);
      float bv = -2.f;                                 // a thread without priors: below every column, retired ones included
      int bi = 0;
      for (int pr = t; pr < p.P; pr += FT) {
        const Box pb = prior_box(p.priors, pr);
        const float ov = forced[pr] >= 0 ? -1.f : iou(gb, ga, pb, area(pb));
        if (ov > bv) { bv = ov; bi = pr; }             // ascending priors: the lowest among equals
      }
      block_argmax(bv, bi, wv, wi);
      if (t == 0) { rmax[r] = bv; rarg[r] = bi; }
    }
    __syncthreads();
  }
}

// smooth-L1 (beta 1) of one prior's four coordinates, and alpha * its derivative
__device__ __forceinline__ float smooth_l1_4(const f32x4 x, const f32x4 tgt, float alpha, f32x4 &g) {
  float l = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float d = x[e] - tgt[e], ad = fabsf(d);
    l += ad < 1.f ? 0.5f * d * d : ad - 0.5f;
    g[e] = alpha * (d < -1.f ? -1.f : (d > 1.f ? 1.f : d));
  }
  return l;
}

// the tile's positives and smooth-L1 sum: a wave butterfly, then the four waves in order
__device__ __forceinline__ void tile_partials(const MtParams &p, bool positive, float l, int b, int tile) {
  __shared__ int cw[4];
  __shared__ float lw[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = ymi_wave_count(positive);
  l = ymi_wave_sum(l);
  if (lane == 0) { cw[wave] = c; lw[wave] = l; }
  __syncthreads();
  if (threadIdx.x == 0) {
    p.ws_cnt[(size_t)b * p.ntiles + tile] = ymi_waves_count<4>(cw);
    p.ws_ls[(size_t)b * p.ntiles + tile] = ymi_waves_sum<4>(lw);
  }
}

__global__ __launch_bounds__(TP) void match_finish_k(const MtParams p) {
  const int t = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
  const int pr = tile * TP + t;
  const bool ok = pr < p.P;
  int g0, n;
  ymi_image_range(p.gt_off, b, p.G, g0, n, p.P);
  bool positive = false;
  float l = 0.f;
  if (ok) {
    const size_t o = (size_t)b * p.P + pr;
    float ov = p.ws_bto[o];
    int idx = p.ws_bti[o];
    const int f = p.ws_forced[o];
    if (f >= 0) { ov = 2.f; idx = f; }                 // box_utils.py:204-207
    int row = g0 + idx;
    row = row > p.G - 1 ? p.G - 1 : row;
    int conf = p.label[row] + 1;
    if (ov < p.pos_thresh) conf = -1;                  // :212-213, in this order
    if (ov < p.neg_thresh) conf = 0;
    if (p.Gc > 0 && p.crowd_thresh < 1.f) {
      int c0, nc;
      ymi_image_range(p.crowd_off, b, p.Gc, c0, nc);
      if (nc > 0 && conf <= 0 && p.ws_bco[o] > p.crowd_thresh) conf = -1;     // :216-222
    }
    const f32x4 m = *reinterpret_cast<const f32x4 *>(p.truth + (size_t)row * 4);
    const f32x4 q = *reinterpret_cast<const f32x4 *>(p.priors + (size_t)pr * 4);
    // encode (box_utils.py:253-263), variances 0.1 and 0.2
    f32x4 lt;
    lt[0] = ((m[0] + m[2]) / 2.f - q[0]) / (0.1f * q[2]);
    lt[1] = ((m[1] + m[3]) / 2.f - q[1]) / (0.1f * q[3]);
    lt[2] = logf((m[2] - m[0]) / q[2]) / 0.2f;
    lt[3] = logf((m[3] - m[1]) / q[3]) / 0.2f;
    positive = conf > 0;
    p.conf_t[o] = conf; p.idx_t[o] = idx; p.pos[o] = positive ? 1 : 0;
    *reinterpret_cast<f32x4 *>(p.gt_box_t + o * 4) = m;
    *reinterpret_cast<f32x4 *>(p.loc_t + o * 4) = lt;
    if (p.loc_data) {
      f32x4 g;
      const float lp = smooth_l1_4(*reinterpret_cast<const f32x4 *>(p.loc_data + o * 4), lt, p.alpha, g);
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      l = positive ? lp : 0.f;
      if (p.d_loc) *reinterpret_cast<f32x4 *>(p.d_loc + o * 4) = positive ? g : zero;
    }
  }
  tile_partials(p, positive, l, b, tile);
}

// the box loss of given targets and positives: the loss half of match_finish_k, the same partial sums
__global__ __launch_bounds__(TP) void box_loss_k(const MtParams p) {
  const int t = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
  const int pr = tile * TP + t;
  bool positive = false;
  float l = 0.f;
  if (pr < p.P) {
    const size_t o = (size_t)b * p.P + pr;
    positive = p.pos_in[o] != 0;
    f32x4 g;
    const float lp = smooth_l1_4(*reinterpret_cast<const f32x4 *>(p.loc_data + o * 4),
                                 *reinterpret_cast<const f32x4 *>(p.loc_t_in + o * 4), p.alpha, g);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    l = positive ? lp : 0.f;
    if (p.d_loc) *reinterpret_cast<f32x4 *>(p.d_loc + o * 4) = positive ? g : zero;
  }
  tile_partials(p, positive, l, b, tile);
}

// one block: num_pos[b] = its tiles' counts in tile order; loss = alpha * the B * ntiles partials, strided sums then a fixed tree
__global__ __launch_bounds__(256) void match_sum_k(const MtParams p) {
  const int t = threadIdx.x;
  if (p.num_pos)
    for (int b = t; b < p.B; b += 256) {
      int c = 0;
      for (int tl = 0; tl < p.ntiles; ++tl) c += p.ws_cnt[(size_t)b * p.ntiles + tl];
      p.num_pos[b] = c;
    }
  if (!p.loss) return;                                 // uniform
  const float s = ymi_sum256(p.ws_ls, (long)p.B * p.ntiles);
  if (t == 0) p.loss[0] = s * p.alpha;
}

int ntiles_of(int P) { return (P + TP - 1) / TP; }

int validate_shape(const ymi_match_desc *d) {
  if (!d) return YMI_ENULL;
  if (d->B < 1 || d->B > 65535 || d->P < 1 || d->G < 1 || d->Gc < 0) return YMI_EARG;
  if (d->P >= (1 << 24) || d->G >= (1 << 24) || d->Gc >= (1 << 24)) return YMI_ESHAPE;
  return YMI_OK;
}

// byte offsets of the workspace parts; returns the total
int64_t layout(const ymi_match_desc *d, int64_t (&off)[10]) {
  const int64_t nt = ntiles_of(d->P), G = d->G, BP = (int64_t)d->B * d->P;
  const int64_t sizes[10] = {nt * G, nt * G, BP, BP, BP, BP, G, G, (int64_t)d->B * nt, (int64_t)d->B * nt};
  return ymi_ws_layout(sizes, off);
}

void bind_ws(MtParams &p, const ymi_match_desc *d, void *ws) {
  int64_t off[10];
  layout(d, off);
  char *w = static_cast<char *>(ws);
  p.ws_pv = (float *)(w + off[0]); p.ws_pi = (int32_t *)(w + off[1]);
  p.ws_bto = (float *)(w + off[2]); p.ws_bti = (int32_t *)(w + off[3]);
  p.ws_bco = (float *)(w + off[4]); p.ws_forced = (int32_t *)(w + off[5]);
  p.ws_rmax = (float *)(w + off[6]); p.ws_rarg = (int32_t *)(w + off[7]);
  p.ws_cnt = (int32_t *)(w + off[8]); p.ws_ls = (float *)(w + off[9]);
}

}  // namespace

extern "C" int64_t ymi_match_ws_bytes(const ymi_match_desc *d) {
  const int rc = validate_shape(d);
  if (rc) return rc;
  int64_t off[10];
  return layout(d, off);
}

// the box loss alone keeps only the per-tile partials: [B][ntiles] counts and sums
extern "C" int64_t ymi_box_loss_ws_bytes(const ymi_match_desc *d) {
  if (!d) return YMI_ENULL;
  if (d->B < 1 || d->B > 65535 || d->P < 1) return YMI_EARG;
  if (d->P >= (1 << 24)) return YMI_ESHAPE;
  return 2 * ymi_ws_part((int64_t)d->B * ntiles_of(d->P));
}

extern "C" int ymi_match_f32(const ymi_match_desc *d, void *stream) {
  const int rc = validate_shape(d);
  if (rc) return rc;
  if (!d->priors || !d->truth || !d->label || !d->gt_off || !d->gt_off_host || !d->loc_t || !d->conf_t || !d->idx_t ||
      !d->gt_box_t || !d->pos || !d->num_pos || !d->ws)
    return YMI_ENULL;
  if (d->Gc > 0 && (!d->crowd || !d->crowd_off || !d->crowd_off_host)) return YMI_ENULL;
  if ((d->d_loc || d->loss) && !d->loc_data) return YMI_EARG;
  if (((uintptr_t)d->priors | (uintptr_t)d->truth | (uintptr_t)d->crowd | (uintptr_t)d->loc_data | (uintptr_t)d->loc_t |
       (uintptr_t)d->gt_box_t | (uintptr_t)d->d_loc | (uintptr_t)d->ws) & 15)
    return YMI_ESHAPE;
  const int rg = ymi_validate_offsets(d->gt_off_host, d->B, d->G, 1, d->P);      // 1 <= n_gt <= P in every image
  if (rg) return rg;
  if (d->Gc > 0) {
    const int rcw = ymi_validate_offsets(d->crowd_off_host, d->B, d->Gc, 0, d->Gc);
    if (rcw) return rcw;
  }

  MtParams p = {};
  p.priors = d->priors; p.truth = d->truth; p.crowd = d->crowd; p.loc_data = d->loc_data;
  p.label = d->label; p.gt_off = d->gt_off; p.crowd_off = d->crowd_off;
  p.loc_t = d->loc_t; p.gt_box_t = d->gt_box_t; p.d_loc = d->d_loc; p.loss = d->loss;
  p.conf_t = d->conf_t; p.idx_t = d->idx_t; p.num_pos = d->num_pos; p.pos = d->pos;
  p.B = d->B; p.P = d->P; p.G = d->G; p.Gc = d->Gc; p.ntiles = ntiles_of(d->P);
  p.pos_thresh = d->pos_thresh; p.neg_thresh = d->neg_thresh; p.crowd_thresh = d->crowd_thresh; p.alpha = d->bbox_alpha;
  bind_ws(p, d, d->ws);

  int rl = ymi_launch(match_best_k, dim3(p.ntiles, d->B), dim3(TP), 0, stream, p);
  if (!rl) rl = ymi_launch(match_force_k, dim3(d->B), dim3(FT), 0, stream, p);
  if (!rl) rl = ymi_launch(match_finish_k, dim3(p.ntiles, d->B), dim3(TP), 0, stream, p);
  if (!rl) rl = ymi_launch(match_sum_k, dim3(1), dim3(256), 0, stream, p);
  return rl;
}

extern "C" int ymi_box_loss_f32(const float *loc_data, const float *loc_t, const uint8_t *pos, int B, int P, float bbox_alpha,
                                float *loss, float *d_loc, void *ws, void *stream) {
  if (!loc_data || !loc_t || !pos || !loss || !ws) return YMI_ENULL;
  if (B < 1 || B > 65535 || P < 1) return YMI_EARG;
  if (P >= (1 << 24)) return YMI_ESHAPE;
  if (((uintptr_t)loc_data | (uintptr_t)loc_t | (uintptr_t)d_loc | (uintptr_t)ws) & 15) return YMI_ESHAPE;
  MtParams p = {};
  p.loc_data = loc_data; p.loc_t_in = loc_t; p.pos_in = pos; p.loss = loss; p.d_loc = d_loc;
  p.B = B; p.P = P; p.ntiles = ntiles_of(P); p.alpha = bbox_alpha;
  p.ws_cnt = static_cast<int32_t *>(ws);
  p.ws_ls = reinterpret_cast<float *>(static_cast<char *>(ws) + ymi_ws_part((int64_t)B * p.ntiles));
  int rl = ymi_launch(box_loss_k, dim3(p.ntiles, B), dim3(TP), 0, stream, p);
  if (!rl) rl = ymi_launch(match_sum_k, dim3(1), dim3(256), 0, stream, p);
  return rl;
}
