// COCO box / mask mAP on device: the bookkeeping half of eval.py's metric mode (prep_metrics, eval.py:445-510; APDataObject.get_ap,
// eval.py:533-581).  The IoU matrices come from csrc/metrics.hip (jaccard_k, mask_iou_bits_k); this file does what the reference does
// with them in Python.
//
// ap_match_k: ONE workgroup per image.  Per detection and per IoU type it writes a record: the type's score, an order key and two
//   10-bit masks (true positive / pushed at threshold k).  eval.py's loops, restated:
//     * type order: box_indices = stable sort by -box score; mask_indices = stable sort OF box_indices by -mask score (ties fall back
//       to the box order, not to the detection index).  Ranks by counting (N <= YMI_AP_MAX_DET), order[t][rank] = detection.
//     * one wave per (type, threshold): walk the detections in the type's order; the lanes scan the unused GT of the detection's
//       class and the wave keeps the largest IoU > the threshold, first j on ties (the reference's strict `iou > max_iou_found`
//       scan from j = 0).  IoUs are fp32 widened to double, thresholds the doubles x / 100.  NaN IoUs never compare greater.
//       gt_used per (class, threshold, type) of the reference = one used-bit per GT per wave: a GT only ever matches detections of
//       its own class.
//     * unmatched: not pushed at this threshold if some crowd region of the class has crowd IoU > threshold.
//   The image's per-class non-crowd GT counts go into gt_count (eval.py:455,462).  An image without detections is never launched
//   (eval.py:405-406 returns before counting its GT).
//   Record keys: (class << 32) | k(score), k ascending = score descending, -0.0 == +0.0.  Records of one image sit at
//   [base, base + N) in the type's order, images in insertion order, so a STABLE sort of the keys gives every (type, class) its
//   data points in the order APDataObject.get_ap's stable sort on -score puts them.
// ap_finalize_k: one wave per (class, type), lane k = threshold k: APDataObject.get_ap in fp64 over the sorted records —
//   precision / recall as int / int divisions, the right-to-left running max, np.searchsorted(recalls, b / 100, 'left') for the 101
//   bars and sum(y_range) / 101 summed left to right.  The bars are found without storing the curve: the first index whose recall
//   reaches b / 100 is the t_b-th true positive, t_b = min{t : t / G >= b / 100} (the division is monotone), so one backward walk
//   carrying the running max fills every bar.
#include "common.h"
#include "../../include/yolact_amd.h"

namespace {

constexpr int NT = YMI_AP_NUM_THRESH;
constexpr int MAXN = YMI_AP_MAX_DET, MAXG = YMI_AP_MAX_GT;
constexpr int MATCH_THREADS = 640;              // 10 waves: each runs 2 of the 20 (type, threshold) walks

__device__ inline double iou_threshold(int k) { return (double)(50 + 5 * k) / 100.0; }     // eval.py:31, x / 100

// ascending order of the result = descending score; -0.0 and +0.0 get the same key
__device__ inline uint32_t desc_score_key(float s) {
  if (s == 0.f) s = 0.f;
  const uint32_t u = __float_as_uint(s);
  return (u & 0x80000000u) ? u : ~(u | 0x80000000u);
}

__global__ __launch_bounds__(MATCH_THREADS) void ap_match_k(ymi_ap_match_desc d) {
  __shared__ float s_bs[MAXN], s_ms[MAXN];
  __shared__ int s_cls[MAXN], s_rank[MAXN];
  __shared__ int s_order[2][MAXN];
  __shared__ int s_flags[2][MAXN];
  __shared__ int s_gcls[MAXG], s_ccls[MAXG];
  const int N = d.N, G = d.G, Gc = d.Gc, C = d.num_classes;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < N; i += MATCH_THREADS) {
    const int64_t c = d.cls[i];
    s_cls[i] = (c >= 0 && c < C) ? (int)c : -1;             // a class outside the table is never pushed
    s_bs[i] = d.box_score[i];
    s_ms[i] = d.mask_score[i];
    s_flags[0][i] = s_flags[1][i] = 0;
  }
  for (int j = tid; j < G; j += MATCH_THREADS) {
    const int c = d.gt_cls[j];
    s_gcls[j] = (c >= 0 && c < C) ? c : -2;
    if (c >= 0 && c < C) atomicAdd((unsigned long long *)&d.gt_count[c], 1ull);
  }
  for (int j = tid; j < Gc; j += MATCH_THREADS) {
    const int c = d.crowd_cls[j];
    s_ccls[j] = (c >= 0 && c < C) ? c : -2;                 // COCO crowds carry class -1: they match no detection
  }
  __syncthreads();
  // box order: stable sort by -box score (ties: detection index)
  for (int i = tid; i < N; i += MATCH_THREADS) {
    const float s = s_bs[i];
    int r = 0;
    for (int j = 0; j < N; ++j) r += (s_bs[j] > s) || (s_bs[j] == s && j < i);
    s_rank[i] = r;
    s_order[0][r] = i;
  }
  __syncthreads();
  // mask order: stable sort of the box order by -mask score (ties: box order)
  for (int i = tid; i < N; i += MATCH_THREADS) {
    const float s = s_ms[i];
    const int rb = s_rank[i];
    int r = 0;
    for (int j = 0; j < N; ++j) r += (s_ms[j] > s) || (s_ms[j] == s && s_rank[j] < rb);
    s_order[1][r] = i;
  }
  __syncthreads();
  for (int combo = wave; combo < 2 * NT; combo += MATCH_THREADS / 64) {
    const int t = combo / NT, k = combo - t * NT;
    const double thr = iou_threshold(k);
    const float *iou = t ? d.mask_iou : d.box_iou;
    const float *ciou = t ? d.crowd_mask_iou : d.crowd_box_iou;
    uint32_t used = 0;                                      // bit ch: GT 64 ch + lane is taken
    for (int p = 0; p < N; ++p) {
      const int i = s_order[t][p];
      const int c = s_cls[i];
      if (c < 0) continue;                                  // wave-uniform
      double best = thr;
      int bj = -1;
      for (int ch = 0; ch * 64 < G; ++ch) {
        const int j = ch * 64 + lane;
        if (j < G && !((used >> ch) & 1u) && s_gcls[j] == c) {
          const double v = (double)iou[(int64_t)i * G + j];
          if (v > best) { best = v; bj = j; }
        }
      }
#pragma unroll
      for (int off = 32; off; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int oj = __shfl_xor(bj, off);
        if (oj >= 0 && (ob > best || (ob == best && (bj < 0 || oj < bj)))) { best = ob; bj = oj; }
      }
      int bits;
      if (bj >= 0) {
        if (lane == (bj & 63)) used |= 1u << (bj >> 6);
        bits = (1 << k) | (1 << (16 + k));
      } else {
        bool hit = false;
        for (int j = lane; j < Gc; j += 64) hit = hit || (s_ccls[j] == c && (double)ciou[(int64_t)i * Gc + j] > thr);
        bits = __ballot(hit) ? 0 : (1 << (16 + k));
      }
      if (lane == 0 && bits) atomicOr(&s_flags[t][p], bits);
    }
  }
  __syncthreads();
  for (int e = tid; e < 2 * N; e += MATCH_THREADS) {
    const int t = e >= N, p = e - t * N;
    const int i = s_order[t][p];
    const float s = t ? s_ms[i] : s_bs[i];
    const int64_t r = (int64_t)t * d.cap + d.base + p;
    d.rec_key[r] = (int64_t)(((uint64_t)(int64_t)s_cls[i] << 32) | desc_score_key(s));
    d.rec_score[r] = s;
    d.rec_flags[r] = s_flags[t][p];
  }
}

__device__ inline int64_t lower_bound(const int64_t *a, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// min{t >= 0 : t / G >= b / 100} in doubles (G >= 1)
__device__ inline int64_t bar_true_count(int b, int64_t G) {
  const double x = (double)b / 100.0, g = (double)G;
  int64_t t = (int64_t)((double)b * g / 100.0);
  if (t < 0) t = 0;
  while (t > 0 && (double)(t - 1) / g >= x) --t;
  while ((double)t / g < x) ++t;
  return t;
}

__global__ __launch_bounds__(64) void ap_finalize_k(ymi_ap_finalize_desc d) {
  __shared__ double y[101][16];
  const int c = blockIdx.x, t = blockIdx.y, k = threadIdx.x;
  if (k >= NT) return;
  int64_t lo = 0, hi = 0;
  if (d.M > 0) {
    const int64_t *key = d.sorted_key + (int64_t)t * d.M;
    lo = lower_bound(key, d.M, (int64_t)c << 32);
    hi = lower_bound(key, d.M, (int64_t)(c + 1) << 32);
  }
  const int64_t *perm = d.perm + (int64_t)t * d.M;
  const int32_t *flags = d.rec_flags + (int64_t)t * d.cap;
  const int64_t G = d.gt_count[c];
  int64_t n = 0, tt = 0;
  for (int64_t r = lo; r < hi; ++r) {
    const int f = flags[perm[r]];
    if ((f >> (16 + k)) & 1) { ++n; tt += (f >> k) & 1; }
  }
  const int64_t o = ((int64_t)t * NT + k) * d.num_classes + c;
  d.empty[o] = (n == 0 && G == 0);                          // APDataObject.is_empty
  if (G == 0) { d.ap[o] = 0.0; return; }                    // get_ap: `if self.num_gt_positives == 0: return 0`
  for (int b = 0; b <= 100; ++b) y[b][k] = 0.0;
  int b = 100;
  while (b >= 0 && bar_true_count(b, G) > tt) --b;          // np.searchsorted ran past the curve: the bar stays 0
  double m = 0.0;
  int64_t i = n - 1, nt = tt;
  for (int64_t r = hi - 1; r >= lo; --r) {
    const int f = flags[perm[r]];
    if (!((f >> (16 + k)) & 1)) continue;
    const double p = (double)nt / (double)(i + 1);          // num_true / (num_true + num_false)
    m = (i == n - 1 || p > m) ? p : m;                      // the smoothing pass: max(precisions[i:])
    if ((f >> k) & 1) {
      while (b >= 1 && bar_true_count(b, G) == nt) { y[b][k] = m; --b; }
      --nt;
    }
    --i;
  }
  if (n > 0)
    for (; b >= 0; --b) y[b][k] = m;                        // recall >= 0 holds at index 0
  double s = 0.0;
  for (int q = 0; q <= 100; ++q) s += y[q][k];              // sum(y_range), left to right
  d.ap[o] = s / 101.0;
}

}  // namespace

extern "C" {

int ymi_ap_match_f32(const ymi_ap_match_desc *d, void *stream) {
  if (!d) return YMI_ENULL;
  if (d->N < 0 || d->G < 0 || d->Gc < 0 || d->num_classes < 1 || d->base < 0 || d->cap < 0) return YMI_EARG;
  if (d->N > YMI_AP_MAX_DET || d->G > YMI_AP_MAX_GT || d->Gc > YMI_AP_MAX_GT || d->base + d->N > d->cap) return YMI_EARG;
  if (d->num_classes > (1 << 30)) return YMI_EARG;
  if (d->N == 0) return 0;                                  // eval.py:405-406: nothing is recorded, not even the GT count
  if (!d->cls || !d->box_score || !d->mask_score || !d->rec_key || !d->rec_score || !d->rec_flags || !d->gt_count) return YMI_ENULL;
  if (d->G > 0 && (!d->box_iou || !d->mask_iou || !d->gt_cls)) return YMI_ENULL;
  if (d->Gc > 0 && (!d->crowd_box_iou || !d->crowd_mask_iou || !d->crowd_cls)) return YMI_ENULL;
  hipLaunchKernelGGL(ap_match_k, dim3(1), dim3(MATCH_THREADS), 0, (hipStream_t)stream, *d);
  return ymi_launch_status();
}

int ymi_ap_finalize_f64(const ymi_ap_finalize_desc *d, void *stream) {
  if (!d) return YMI_ENULL;
  if (d->M < 0 || d->cap < d->M || d->num_classes < 1 || d->num_classes > 65535) return YMI_EARG;
  if (!d->gt_count || !d->ap || !d->empty) return YMI_ENULL;
  if (d->M > 0 && (!d->sorted_key || !d->perm || !d->rec_flags)) return YMI_ENULL;
  hipLaunchKernelGGL(ap_finalize_k, dim3(d->num_classes, 2), dim3(64), 0, (hipStream_t)stream, *d);
  return ymi_launch_status();
}

}  // extern "C"
