// Detect with traditional (greedy, per-class) NMS on device: the reference's use_fast_nms = False mode.
// Reference: layers/functions/detection.py:80-108,182-228 (Detect.detect / traditional_nms), utils/cython_nms.pyx:24-74 (nms),
//            layers/box_utils.py:267-312 (decode).
//
// Whole batch in three launches, no host synchronisation, fixed-capacity outputs + counts (cap = max_det):
//   G1  grid (P/64, B)      softmax over C classes (the op order of detect.hip's first stage), class-major scores [B,C-1,P],
//                           decoded boxes times box_scale (cfg.max_size) [B,P,4]
//   G2  grid (C-1, B)       1024 threads, one block per (class, image): compact the candidates (score > conf_thresh) in prior
//                           order, sort them (score desc, prior asc) with a bitonic network, run the greedy pass, write the best
//                           max_det survivors of the class
//   G3  grid (B)            1024 threads: sort all per-class survivors of an image (score desc, class asc, prior asc), write the
//                           best max_det
// Candidate keys live in LDS when a class has at most KLDS of them (the common case), otherwise in the caller's global workspace
// (one [P] slice per (image, class)): the same code on the other address space, never a truncation.
// Greedy pass: the sorted candidates are taken in chunks of 64.  Every candidate of a chunk is first tested against all survivors
// so far (1024 threads: 64 candidates x 16 survivor stripes), then the chunk is resolved inside itself by one wave: lane l holds
// the 64-bit mask of the later chunk members l suppresses, and a scalar walk over the survivors of the chunk clears them.
// Overlap exactly as cython_nms.pyx evaluates it, in pixels with the "+1" convention: area = (x2-x1+1)*(y2-y1+1),
// w = max(0, xx2-xx1+1), ovr = inter / (iarea + area_j - inter), suppressed when ovr >= nms_thresh.  Build with -ffp-contract=off;
// the division is IEEE (correctly rounded).
// Tie rule (the reference's argsort / torch.sort are unstable, so its order of exactly tied scores is not defined): score desc,
// then class asc, then prior asc.
#include "detect_common.h"
#include "../../include/yolact_amd.h"

namespace {

constexpr int GNT = 1024;        // threads of G2 / G3
constexpr int KLDS = 4096;       // candidate keys per class held in LDS (32 KiB); more go to the global workspace
constexpr int SLDS = 2048;       // survivor boxes cached in LDS (32 KiB); later survivors are read back from the box array
constexpr int MLDS = 8192;       // G3: per-image survivor keys sorted in LDS (64 KiB); more are sorted in place in the workspace
constexpr int CAP_MAX = 256;     // max_det limit (as ymi_detect_f32)

// cython_nms.pyx's max / min (first operand on ties) and its overlap test; `a` is the higher-ranked box
__device__ __forceinline__ float cmax(float a, float b) { return a >= b ? a : b; }
__device__ __forceinline__ float cmin(float a, float b) { return a <= b ? a : b; }
__device__ __forceinline__ float area1(const f32x4 a) { return ((a[2] - a[0]) + 1.f) * ((a[3] - a[1]) + 1.f); }
__device__ __forceinline__ bool ovr_ge(const f32x4 a, const f32x4 b, float thresh) {
  const float xx1 = cmax(a[0], b[0]), yy1 = cmax(a[1], b[1]);
  const float xx2 = cmin(a[2], b[2]), yy2 = cmin(a[3], b[3]);
  const float w = cmax(0.f, (xx2 - xx1) + 1.f), h = cmax(0.f, (yy2 - yy1) + 1.f);
  const float inter = w * h;
  const float ovr = inter / ((area1(a) + area1(b)) - inter);
  return ovr >= thresh;
}

__device__ __forceinline__ int key_prior(unsigned long long k) { return (int)(0xffffffffu - (unsigned)(k & 0xffffffffull)); }

// Bitonic sort of kb[0..n) DESCENDING, n arbitrary: the network of the next power of two in its "flip" form (every compare-exchange
// puts the larger key at the lower index), so the virtual elements past n (minimal keys) never move and are simply skipped.
// kb: LDS or global, owned by this block.
template <typename KeyPtr>
__device__ void block_sort_desc(KeyPtr kb, int n) {
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  const int t = threadIdx.x;
  for (int size = 2; size <= n2; size <<= 1) {
    const int half = size >> 1;
    for (int q = t; q < (n2 >> 1); q += GNT) {
      const int blk = q / half, off = q - blk * half;
      const int i = blk * size + off, j = blk * size + size - 1 - off;
      if (j < n) {
        const unsigned long long a = kb[i], c = kb[j];
        if (c > a) { kb[i] = c; kb[j] = a; }
      }
    }
    __syncthreads();
    for (int s = size >> 2; s > 0; s >>= 1) {
      for (int q = t; q < (n2 >> 1); q += GNT) {
        const int i = (q / s) * 2 * s + (q % s), j = i + s;
        if (j < n) {
          const unsigned long long a = kb[i], c = kb[j];
          if (c > a) { kb[i] = c; kb[j] = a; }
        }
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------------------
// G1: softmax (detect.hip softmax_keep_k's op order) + class-major scores + pixel-scale boxes.  Block = 64 priors x C classes in LDS.
__global__ __launch_bounds__(256) void greedy_prep_k(const float *__restrict__ conf, const float *__restrict__ loc,
                                                     const float *__restrict__ priors, int P, int C, int ld, int is_logits,
                                                     float box_scale, float *__restrict__ scores_t, f32x4 *__restrict__ pixbox) {
  extern __shared__ float s[];  // 64 * C
  const int b = blockIdx.y, p0 = blockIdx.x * 64;
  const int np = min(64, P - p0);
  const int t = threadIdx.x;
  const float *src = conf + ((size_t)b * P + p0) * ld;
  for (int i = t; i < np * C; i += 256) { const int jj = i / C, c = i - jj * C; s[i] = src[(size_t)jj * ld + c]; }
  if (t < np) {
    const int p = p0 + t;
    const f32x4 bb = decode_box(loc + ((size_t)b * P + p) * 4, priors + (size_t)p * 4);
    f32x4 o;
    o[0] = bb[0] * box_scale; o[1] = bb[1] * box_scale; o[2] = bb[2] * box_scale; o[3] = bb[3] * box_scale;
    pixbox[(size_t)b * P + p] = o;
  }
  __syncthreads();
  if (is_logits) {
    const int j = t >> 2, sub = t & 3;  // 4 lanes per prior
    float *row = s + j * C;
    const bool live = j < np;
    float mx = -__builtin_inff();
    if (live) for (int c = sub; c < C; c += 4) mx = fmaxf(mx, row[c]);
    mx = fmaxf(mx, __shfl_xor(mx, 1));
    mx = fmaxf(mx, __shfl_xor(mx, 2));
    float sum = 0.f;
    if (live) for (int c = sub; c < C; c += 4) { const float e = expf(row[c] - mx); row[c] = e; sum += e; }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    if (live) for (int c = sub; c < C; c += 4) row[c] = row[c] / sum;
    __syncthreads();
  }
  const int nfg = C - 1;
  for (int i = t; i < nfg * 64; i += 256) {
    const int c = i >> 6, jj = i & 63;
    if (jj < np) scores_t[((size_t)b * nfg + c) * P + p0 + jj] = s[jj * C + c + 1];
  }
}

// ------------------------------------------------------------------------------------------------
// G2 body on one key buffer (LDS or the global slice): compact, sort, greedy; returns the survivor count (block-uniform) and leaves
// the survivors' keys, in rank order, in kb[0..ns).
struct GreedyShared {
  f32x4 sbox[SLDS];          // boxes of the first SLDS survivors
  f32x4 cbox[64];            // boxes of the current chunk
  unsigned long long ckey[64];
  unsigned wave_cnt[GNT / 64];
  int presup[64];            // chunk member suppressed by an earlier survivor
  int ns;
};

template <typename KeyPtr>
__device__ int greedy_class(KeyPtr kb, int K, const float *sc, const f32x4 *box, int P, float conf_thresh, float nms_thresh,
                            GreedyShared &sh) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  // compaction in prior order: one tile of GNT priors per step, ballot ranks inside a wave, wave totals through LDS
  int run = 0;
  for (int base = 0; base < P; base += GNT) {
    const int p = base + t;
    const float v = p < P ? sc[p] : 0.f;
    const bool cand = p < P && v > conf_thresh;
    const unsigned long long m = __ballot(cand);
    if (lane == 0) sh.wave_cnt[w] = (unsigned)__popcll(m);
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int ww = 0; ww < GNT / 64; ++ww) { const int x = (int)sh.wave_cnt[ww]; if (ww < w) before += x; tot += x; }
    if (cand) {
      const int pos = run + before + __popcll(m & ((1ull << lane) - 1ull));
      kb[pos] = ((unsigned long long)f2key(v) << 32) | (unsigned)(0xffffffffu - (unsigned)p);
    }
    run += tot;
    __syncthreads();
  }
  block_sort_desc(kb, K);

  if (t < 64) sh.presup[t] = 0;
  if (t == 0) sh.ns = 0;
  __syncthreads();
  int ns = 0;
  const int j = lane, stripe = w;
  for (int i0 = 0; i0 < K; i0 += 64) {
    const int m = min(64, K - i0);
    if (t < m) {
      const unsigned long long k = kb[i0 + t];
      sh.ckey[t] = k;
      sh.cbox[t] = box[key_prior(k)];
    }
    __syncthreads();
    // every chunk member against every survivor so far (survivors outrank the whole chunk)
    if (j < m && ns > 0) {
      const f32x4 bj = sh.cbox[j];
      bool sup = false;
      for (int s = stripe; s < ns && !sup; s += GNT / 64) {
        const f32x4 bs = s < SLDS ? sh.sbox[s] : box[key_prior(kb[s])];
        sup = ovr_ge(bs, bj, nms_thresh);
      }
      if (sup) sh.presup[j] = 1;
    }
    __syncthreads();
    if (t < 64) {
      // inside the chunk: lane l's mask of the later members it suppresses, then a walk over the live members in rank order
      unsigned long long row = 0;
      if (lane < m) {
        const f32x4 bl = sh.cbox[lane];
        for (int jj = lane + 1; jj < m; ++jj)
          if (ovr_ge(bl, sh.cbox[jj], nms_thresh)) row |= 1ull << jj;
      }
      unsigned long long alive = __ballot(lane < m && sh.presup[lane] == 0);
      unsigned long long todo = alive;
      while (todo) {
        const int ii = __builtin_ctzll(todo);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)row, ii);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(row >> 32), ii);
        alive &= ~(((unsigned long long)hi << 32) | lo);
        todo = alive & ~((2ull << ii) - 1ull);           // (ii = 63: 2ull << 63 wraps to 0, todo = 0)
      }
      if ((alive >> lane) & 1ull) {
        // positions ns.. < i0 + 64: every key there has already been copied to ckey
        const int pos = ns + __popcll(alive & ((1ull << lane) - 1ull));
        kb[pos] = sh.ckey[lane];
        if (pos < SLDS) sh.sbox[pos] = sh.cbox[lane];
      }
      sh.presup[lane] = 0;
      if (lane == 0) sh.ns = ns + __popcll(alive);
    }
    __syncthreads();
    ns = sh.ns;
  }
  return ns;
}

// G2: one block per (class, image).  Writes the best min(ns, max_det) survivors of the class to the image's merge keys
// (score key << 32 | ~flat index, flat index = class * max_det + rank; 0 = empty) and their prior indices.
__global__ __launch_bounds__(GNT) void greedy_class_k(const float *__restrict__ scores_t, const f32x4 *__restrict__ pixbox,
                                                      int P, int nfg, int max_det, float conf_thresh, float nms_thresh,
                                                      unsigned long long *__restrict__ sort_ws, unsigned long long *__restrict__ cand_key,
                                                      int *__restrict__ cand_prior) {
  __shared__ GreedyShared sh;
  __shared__ unsigned long long kl[KLDS];
  __shared__ unsigned cnt_w[GNT / 64];
  const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const float *sc = scores_t + ((size_t)b * nfg + c) * P;
  const f32x4 *box = pixbox + (size_t)b * P;
  // K = candidates of this class
  unsigned cnt = 0;
  for (int p = t; p < P; p += GNT) cnt += sc[p] > conf_thresh ? 1u : 0u;
  for (int off = 32; off > 0; off >>= 1) cnt += (unsigned)__shfl_xor((int)cnt, off);
  if ((t & 63) == 0) cnt_w[t >> 6] = cnt;
  __syncthreads();
  int K = 0;
#pragma unroll
  for (int ww = 0; ww < GNT / 64; ++ww) K += (int)cnt_w[ww];
  int ns = 0;
  unsigned long long *kg = sort_ws + ((size_t)b * nfg + c) * P;
  if (K > 0) {
    if (K <= KLDS) ns = greedy_class(kl, K, sc, box, P, conf_thresh, nms_thresh, sh);
    else ns = greedy_class(kg, K, sc, box, P, conf_thresh, nms_thresh, sh);
  }
  const int nout = min(ns, max_det);
  unsigned long long *ck = cand_key + (size_t)b * nfg * max_det;
  int *cp = cand_prior + (size_t)b * nfg * max_det;
  for (int r = t; r < max_det; r += GNT) {
    const int f = c * max_det + r;
    if (r < nout) {
      const unsigned long long k = K <= KLDS ? kl[r] : kg[r];
      ck[f] = (k & 0xffffffff00000000ull) | (unsigned)(0xffffffffu - (unsigned)f);
      cp[f] = key_prior(k);
    } else {
      ck[f] = 0ull;
      cp[f] = -1;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// G3: one block per image: the best max_det of all per-class survivors, outputs and the packed record (as ymi_detect_f32 writes them)
__global__ __launch_bounds__(GNT) void greedy_merge_k(unsigned long long *__restrict__ cand_key, const int *__restrict__ cand_prior,
                                                      const f32x4 *__restrict__ pixbox, const float *__restrict__ coef, int P, int D,
                                                      int nfg, int max_det, float box_scale, int *__restrict__ out_count,
                                                      float *__restrict__ out_box, float *__restrict__ out_score,
                                                      long long *__restrict__ out_class, float *__restrict__ out_coef,
                                                      int *__restrict__ out_prior, float *__restrict__ out_rec) {
  __shared__ unsigned long long ml[MLDS];
  __shared__ int sel_prior[CAP_MAX];
  __shared__ unsigned nvalid;
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = nfg * max_det, cap = max_det;
  unsigned long long *ck = cand_key + (size_t)b * n;
  const int *cp = cand_prior + (size_t)b * n;
  const int RL = 6 + D;
  float *rec = out_rec ? out_rec + (size_t)b * (1 + (size_t)cap * RL) : nullptr;
  if (t == 0) nvalid = 0;
  __syncthreads();
  unsigned local = 0;
  const bool in_lds = n <= MLDS;
  for (int i = t; i < n; i += GNT) {
    const unsigned long long k = ck[i];
    local += k != 0ull ? 1u : 0u;
    if (in_lds) ml[i] = k;
  }
  if (local) atomicAdd(&nvalid, local);
  __syncthreads();
  const int k = min((int)nvalid, cap);
  if (t == 0) { out_count[b] = k; if (rec) rec[0] = (float)k; }
  if (k == 0) return;
  if (in_lds) block_sort_desc(ml, n);
  else block_sort_desc(ck, n);
  for (int j = t; j < k; j += GNT) {
    const unsigned long long key = in_lds ? ml[j] : ck[j];
    const int f = key_prior(key);                    // (the low word holds ~flat index)
    const int cls = f / max_det;
    const int prior = cp[f];
    sel_prior[j] = prior;
    const float sv = key2f((unsigned)(key >> 32));
    const f32x4 pb = pixbox[(size_t)b * P + prior];
    f32x4 bb;                                        // detection.py:228: (boxes * max_size)[idx] / max_size
    bb[0] = pb[0] / box_scale; bb[1] = pb[1] / box_scale; bb[2] = pb[2] / box_scale; bb[3] = pb[3] / box_scale;
    float *ob = out_box + ((size_t)b * cap + j) * 4;
    ob[0] = bb[0]; ob[1] = bb[1]; ob[2] = bb[2]; ob[3] = bb[3];
    out_score[(size_t)b * cap + j] = sv;
    out_class[(size_t)b * cap + j] = cls;
    out_prior[(size_t)b * cap + j] = prior;
    if (rec) {
      float *r = rec + 1 + (size_t)j * RL;
      r[0] = bb[0]; r[1] = bb[1]; r[2] = bb[2]; r[3] = bb[3]; r[4] = sv; r[5] = (float)cls;
    }
  }
  __syncthreads();
  for (int i = t; i < k * D; i += GNT) {
    const int j = i / D, e = i - j * D;
    const float cv = coef[((size_t)b * P + sel_prior[j]) * D + e];
    out_coef[((size_t)b * cap + j) * D + e] = cv;
    if (rec) rec[1 + (size_t)j * RL + 6 + e] = cv;
  }
}

}  // namespace

// Workspace layout of ymi_detect_greedy_ws.ws (ymi_workspace_bytes(YMI_WS_DETECT_GREEDY)): pixel boxes [B,P] f32x4 | merge keys
// [B,(C-1)*max_det] u64 | their priors [B,(C-1)*max_det] i32 | large-K candidate keys [B,C-1,P] u64; each part 256-byte aligned.
extern "C" __attribute__((visibility("hidden"))) int64_t ymi_detect_greedy_layout(const ymi_detect_desc *d, int64_t off[4]) {
  auto al = [](int64_t x) { return (x + 255) / 256 * 256; };
  const int64_t B = d->B, P = d->P, nfg = d->C - 1, M = d->max_det;
  off[0] = 0;
  off[1] = al(off[0] + 16 * B * P);
  off[2] = al(off[1] + 8 * B * nfg * M);
  off[3] = al(off[2] + 4 * B * nfg * M);
  return al(off[3] + 8 * B * nfg * P);
}

extern "C" int ymi_detect_traditional_f32(const ymi_detect_desc *d, const ymi_detect_greedy_ws *g, void *stream) {
  if (!d || !g) return YMI_ENULL;
  if (!d->conf || !d->loc || !d->coef || !d->priors || !d->scores_t || !g->ws || !d->out_count || !d->out_box || !d->out_score ||
      !d->out_class || !d->out_coef || !d->out_prior)
    return YMI_ENULL;
  if (d->B <= 0 || d->P <= 0 || d->C < 2 || d->D <= 0 || (d->conf_ld != 0 && d->conf_ld < d->C)) return YMI_EARG;
  if (d->max_det <= 0 || d->max_det > CAP_MAX || d->B > 65535 || d->C - 1 > 65535) return YMI_EARG;
  if (!(g->box_scale > 0.f)) return YMI_EARG;
  if ((size_t)64 * d->C * sizeof(float) > 60000) return YMI_ESHAPE;
  // key encodings: prior index and flat survivor index in 32 bits, bitonic index arithmetic in int
  if ((int64_t)d->P >= (1ll << 30) || (int64_t)(d->C - 1) * d->max_det >= (1ll << 30)) return YMI_ESHAPE;
  int64_t off[4];
  ymi_detect_greedy_layout(d, off);
  char *ws = (char *)g->ws;
  f32x4 *pixbox = (f32x4 *)(ws + off[0]);
  unsigned long long *cand_key = (unsigned long long *)(ws + off[1]);
  int *cand_prior = (int *)(ws + off[2]);
  unsigned long long *sort_ws = (unsigned long long *)(ws + off[3]);
  if (((uintptr_t)ws) & 15) return YMI_ESHAPE;
  hipStream_t s = (hipStream_t)stream;
  const int nfg = d->C - 1;
  hipLaunchKernelGGL(greedy_prep_k, dim3((d->P + 63) / 64, d->B), dim3(256), 64 * d->C * sizeof(float), s, d->conf, d->loc,
                     d->priors, d->P, d->C, d->conf_ld > 0 ? d->conf_ld : d->C, d->conf_is_logits, g->box_scale, d->scores_t,
                     pixbox);
  int rc = ymi_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(greedy_class_k, dim3(nfg, d->B), dim3(GNT), 0, s, d->scores_t, pixbox, d->P, nfg, d->max_det,
                     d->conf_thresh, d->nms_thresh, sort_ws, cand_key, cand_prior);
  rc = ymi_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(greedy_merge_k, dim3(d->B), dim3(GNT), 0, s, cand_key, cand_prior, pixbox, d->coef, d->P, d->D, nfg,
                     d->max_det, g->box_scale, d->out_count, d->out_box, d->out_score, (long long *)d->out_class, d->out_coef,
                     d->out_prior, d->out_rec);
  return ymi_launch_status();
}
