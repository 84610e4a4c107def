// COCO ground-truth masks rasterised on the device: every annotation of an image, or of a batch of images, in one launch.
// Byte-equal to the host codec csrc/coco_host.cpp (pycocotools' rleFrPoly / rleDecode restated); the contract, the error codes
// and the algorithm are the comment of ymi_coco_masks_u8 in include/yolact_amd.h.
//
// LIMIT: h * w <= YMI_COCO_MASK_MAX_PIXELS = 640000 pixels (800 x 800) per annotation: two bitmaps of h w + 1 bits in the 160 KiB
// of LDS of one workgroup.  Above it the entry returns YMI_EUNSUPPORTED and the caller rasterises that annotation on the host.
//
// Why a bitmap and no sort.  The host walks the 5x upsampled boundary point by point, emits the column-major position
// q = x h + y of every qualifying change of u, sorts the positions and merges zero-length runs.  Pairs of equal positions cancel
// and the runs alternate from 0, so mask[q] = parity(#positions <= q) over the COLUMN-major flattening -- and the parity runs across
// column ends (a crossing clamped to yd = h lands on (x + 1) h; an odd column carries into the next one), so the scan below is
// over the whole bitmap, never per column.  Positions commute under XOR: integer atomicXor on LDS words, the same bits on every run.
//
// Thread mapping: one workgroup of 1024 threads per annotation, looping over its polygons.  A wave takes an edge, its lanes the
// points d, d + 64, ... of that edge; each point recomputes its predecessor.  The prefix XOR gives every thread a run of
// consecutive words; the transposition gives every thread four consecutive output bytes (one 4-byte store).
//
// -ffp-contract=off (the Makefile's flag, and the pragma below): a fused ys + s * t changes which pixel an edge rounds to.
#include "common.h"
#include "../../include/yolact_amd.h"
#include <cmath>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 1024, kWaves = kBlock / 64;

struct CocoParams {
  const ymi_coco_mask_rec *recs;   // device [n]
  const double *xy;                // device
  const int32_t *poly_len;         // device
  const uint32_t *counts;          // device
  int n;
};

// one edge of the closed polygon, as coco_host.cpp sets it up before its inner loop
struct Edge {
  int xs, ys, dmax;
  bool flip, wide;   // wide: dx >= dy (u steps, v interpolated)
  double s;
};

__device__ __forceinline__ int scaled(double v) { return (int)(5.0 * v + .5); }

__device__ __forceinline__ Edge make_edge(const double *xy, int k, int j) {
  const int j1 = j + 1 == k ? 0 : j + 1;
  int xs = scaled(xy[2 * j]), ys = scaled(xy[2 * j + 1]), xe = scaled(xy[2 * j1]), ye = scaled(xy[2 * j1 + 1]);
  const int dx = abs(xe - xs), dy = abs(ys - ye);
  Edge e;
  e.flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
  if (e.flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
  e.wide = dx >= dy;
  if (e.wide) {
    e.s = dx ? (double)(ye - ys) / dx : 0.0;
    e.dmax = dx;
  } else {
    e.s = (double)(xe - xs) / dy;
    e.dmax = dy;
  }
  e.xs = xs; e.ys = ys;
  return e;
}

__device__ __forceinline__ void edge_point(const Edge &e, int d, int &u, int &v) {
  const int t = e.flip ? e.dmax - d : d;
  if (e.wide) {
    u = t + e.xs;
    v = (int)(e.ys + e.s * t + .5);
  } else {
    v = t + e.ys;
    u = (int)(e.xs + e.s * t + .5);
  }
}

__device__ __forceinline__ void toggle(uint32_t *bits, uint32_t q, uint32_t total) {
  if (q <= total) atomicXor(&bits[q >> 5], 1u << (q & 31u));
}

// the host's "points along the y-boundary" for one point (u, v) and its predecessor (pu, pv)
__device__ __forceinline__ void crossing(int u, int v, int pu, int pv, int h, int w, uint32_t *bits) {
  if (u == pu) return;
  double xd = (double)(u < pu ? u : u - 1);
  xd = (xd + .5) / 5.0 - .5;
  if (floor(xd) != xd || xd < 0 || xd > w - 1) return;
  double yd = (double)(v < pv ? v : pv);
  yd = (yd + .5) / 5.0 - .5;
  if (yd < 0) yd = 0;
  else if (yd > h) yd = h;
  yd = ceil(yd);
  toggle(bits, (uint32_t)((int)xd * h + (int)yd), (uint32_t)h * (uint32_t)w);
}

__device__ void toggle_polygon(const double *xy, int k, int h, int w, uint32_t *bits) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int j = wave; j < k; j += kWaves) {
    const Edge e = make_edge(xy, k, j);
    for (int d = lane; d <= e.dmax; d += 64) {
      int u, v, pu, pv;
      edge_point(e, d, u, v);
      if (d > 0) edge_point(e, d - 1, pu, pv);
      else if (j > 0) {
        const Edge p = make_edge(xy, k, j - 1);     // the previous edge's last point
        edge_point(p, p.dmax, pu, pv);
      } else continue;                              // the walk's first point has no predecessor
      crossing(u, v, pu, pv, h, w, bits);
    }
  }
}

// exclusive prefix sum of one value per thread over the block; scratch [kWaves]
__device__ __forceinline__ uint32_t block_exclusive_sum(uint32_t v, uint32_t *scratch) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) scratch[wave] = inc;
  __syncthreads();
  uint32_t base = 0;
  for (int i = 0; i < wave; ++i) base += scratch[i];
  __syncthreads();
  return base + inc - v;
}

// the boundaries between runs are the prefix sums of the counts: toggle them, the prefix XOR below fills the odd runs
__device__ void toggle_counts(const uint32_t *cnt, int n, uint32_t total, uint32_t *bits, uint32_t *scratch) {
  const int per = (n + kBlock - 1) / kBlock;
  const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
  uint32_t sum = 0;
  for (int i = lo; i < hi; ++i) sum += cnt[i];
  uint32_t pos = block_exclusive_sum(sum, scratch);
  for (int i = lo; i < hi; ++i) {
    pos += cnt[i];
    toggle(bits, pos, total);
  }
}

// bits := inclusive prefix XOR of bits over all nw words; uni |= bits
__device__ void prefix_xor_into(uint32_t *bits, uint32_t *uni, int nw, uint32_t *scratch) {
  const int per = (nw + kBlock - 1) / kBlock;
  const int lo = min(nw, (int)threadIdx.x * per), hi = min(nw, lo + per);
  uint32_t carry = 0;
  for (int i = lo; i < hi; ++i) {
    uint32_t x = bits[i];
    x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;
    x ^= carry;
    bits[i] = x;
    carry = 0u - (x >> 31);
  }
  const uint32_t inv = 0u - (block_exclusive_sum(carry & 1u, scratch) & 1u);   // the parity of everything before this thread's words
  for (int i = lo; i < hi; ++i) uni[i] |= bits[i] ^ inv;
}

__device__ __forceinline__ uint32_t mask_bit(const uint32_t *uni, uint32_t x, uint32_t y, uint32_t h) {
  const uint32_t q = x * h + y;
  return (uni[q >> 5] >> (q & 31u)) & 1u;
}

// W: words of one bitmap (LDS = 2 W words); one workgroup per record
template <int W>
__global__ __launch_bounds__(kBlock) void coco_mask_k(const CocoParams p) {
  __shared__ uint32_t lds[2 * W];
  __shared__ uint32_t scratch[kWaves];
  for (int a = blockIdx.x; a < p.n; a += gridDim.x) {
    const ymi_coco_mask_rec r = p.recs[a];
    const uint32_t h = (uint32_t)r.h, w = (uint32_t)r.w, total = h * w;
    const int nw = (int)((total + 32u) >> 5);          // h w + 1 bits
    if (nw > W) continue;                              // (the host has checked: never taken)
    uint32_t *bits = lds, *uni = lds + W;
    for (int i = threadIdx.x; i < nw; i += kBlock) uni[i] = 0u;
    __syncthreads();                                   // (an empty polygon list goes straight to the transposition)
    const int pieces = r.kind == YMI_COCO_POLY ? r.n : 1;
    int vert = r.xy_first;
    for (int piece = 0; piece < pieces; ++piece) {
      for (int i = threadIdx.x; i < nw; i += kBlock) bits[i] = 0u;
      __syncthreads();
      if (r.kind == YMI_COCO_POLY) {
        const int k = p.poly_len[r.first + piece];
        toggle_polygon(p.xy + 2 * (int64_t)vert, k, r.h, r.w, bits);
        vert += k;
      } else {
        toggle_counts(p.counts + r.first, r.n, total, bits, scratch);
      }
      __syncthreads();
      prefix_xor_into(bits, uni, nw, scratch);
      __syncthreads();
    }
    // column-major bits -> row-major bytes: single bytes up to a 4-byte boundary of `out`, then one 4-byte store per thread
    uint8_t *out = r.out;
    uint32_t lead = (uint32_t)((4u - (uint32_t)((uintptr_t)out & 3u)) & 3u);
    if (lead > total) lead = total;
    const uint32_t body = (total - lead) >> 2, tail0 = lead + 4u * body;
    for (uint32_t i = threadIdx.x; i < lead; i += kBlock) out[i] = (uint8_t)mask_bit(uni, i % w, i / w, h);
    for (uint32_t i = threadIdx.x; i < body; i += kBlock) {
      const uint32_t first = lead + 4u * i;
      uint32_t y = first / w, x = first - y * w, v = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        v |= mask_bit(uni, x, y, h) << (8 * b);
        if (++x == w) { x = 0; ++y; }
      }
      *reinterpret_cast<uint32_t *>(out + first) = v;
    }
    for (uint32_t i = tail0 + threadIdx.x; i < total; i += kBlock) out[i] = (uint8_t)mask_bit(uni, i % w, i / w, h);
    __syncthreads();
  }
}

inline int64_t pad16(int64_t x) { return (x + 15) / 16 * 16; }

// fill_runs' checks (csrc/coco_host.cpp) without the fill
int check_counts(const uint32_t *cnt, int64_t n, int64_t total) {
  int64_t pos = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (pos + (int64_t)cnt[i] > total) return YMI_EFORMAT;
    pos += cnt[i];
  }
  return pos == total ? YMI_OK : YMI_EFORMAT;
}

template <int W>
void launch(const CocoParams &p, hipStream_t s) {
  hipLaunchKernelGGL(coco_mask_k<W>, dim3((unsigned)(p.n < 65535 ? p.n : 65535)), dim3(kBlock), 0, s, p);
}

// bitmap words of the largest record -> the smallest kernel that holds it (the last one: YMI_COCO_MASK_MAX_PIXELS + 1 bits)
constexpr int kW0 = 1024, kW1 = 4096, kW2 = 10240, kW3 = (YMI_COCO_MASK_MAX_PIXELS + 32) / 32;
static_assert((2 * kW3 + kWaves) * 4 <= 160 * 1024, "two bitmaps and the scan scratch in one workgroup's LDS");

}  // namespace

// vertices [n_vert,2] doubles | records [n] | polygon lengths [n_poly] | counts [n_counts], each part padded to 16 bytes
extern "C" __attribute__((visibility("hidden"))) int64_t ymi_coco_mask_ws_bytes(const ymi_coco_mask_desc *d) {
  if (!d || d->n < 1 || d->n_vert < 0 || d->n_poly < 0 || d->n_counts < 0) return YMI_EARG;
  return pad16(d->n_vert * 16) + pad16((int64_t)d->n * (int64_t)sizeof(ymi_coco_mask_rec)) + pad16(d->n_poly * 4) + pad16(d->n_counts * 4);
}

extern "C" int ymi_coco_masks_u8(const ymi_coco_mask_desc *d, void *stream) {
  if (!d || !d->recs || !d->ws) return YMI_ENULL;
  if (d->n < 1 || d->n_vert < 0 || d->n_poly < 0 || d->n_counts < 0) return YMI_EARG;
  if (d->n_vert >= (1LL << 30) || d->n_poly >= (1LL << 31) || d->n_counts >= (1LL << 31)) return YMI_ESHAPE;
  int64_t max_pixels = 0;
  bool over_cap = false;
  for (int i = 0; i < d->n; ++i) {
    const ymi_coco_mask_rec &r = d->recs[i];
    if (!r.out) return YMI_ENULL;
    if (r.h <= 0 || r.w <= 0 || (int64_t)r.h * r.w > (1LL << 31) - 1) return YMI_EARG;
    const int64_t total = (int64_t)r.h * r.w;
    if (r.kind == YMI_COCO_POLY) {
      if (r.n > 0 && (!d->xy || !d->poly_len)) return YMI_ENULL;
      if (r.n < 0) return YMI_EARG;
      if (r.first < 0 || (int64_t)r.first + r.n > d->n_poly || r.xy_first < 0) return YMI_ESHAPE;
      const double lim = 3.0 * (r.w > r.h ? r.w : r.h) + 1024.0;
      int64_t vert = r.xy_first;
      for (int q = 0; q < r.n; ++q) {
        const int k = d->poly_len[r.first + q];
        if (k < 1) return YMI_EARG;
        if (vert + k > d->n_vert) return YMI_ESHAPE;
        for (int64_t j = 2 * vert; j < 2 * (vert + k); ++j) if (!(std::fabs(d->xy[j]) <= lim)) return YMI_EARG;
        vert += k;
      }
    } else if (r.kind == YMI_COCO_COUNTS) {
      if (r.n < 0) return YMI_EARG;
      if (r.n > 0 && !d->counts) return YMI_ENULL;
      if (r.first < 0 || (int64_t)r.first + r.n > d->n_counts) return YMI_ESHAPE;
      const int rc = check_counts(d->counts + r.first, r.n, total);
      if (rc != YMI_OK) return rc;
    } else {
      return YMI_EARG;
    }
    if (total > YMI_COCO_MASK_MAX_PIXELS) over_cap = true;
    if (total > max_pixels) max_pixels = total;
  }
  const int64_t xy_bytes = pad16(d->n_vert * 16), rec_bytes = pad16((int64_t)d->n * (int64_t)sizeof(ymi_coco_mask_rec));
  const int64_t len_bytes = pad16(d->n_poly * 4), need = ymi_coco_mask_ws_bytes(d);
  if (d->ws_bytes < need || ((uintptr_t)d->ws & 15)) return YMI_ESHAPE;
  if (over_cap) return YMI_EUNSUPPORTED;

  std::vector<unsigned char> table((size_t)need, 0);
  if (d->n_vert) std::memcpy(table.data(), d->xy, (size_t)d->n_vert * 16);
  std::memcpy(table.data() + xy_bytes, d->recs, (size_t)d->n * sizeof(ymi_coco_mask_rec));
  if (d->n_poly) std::memcpy(table.data() + xy_bytes + rec_bytes, d->poly_len, (size_t)d->n_poly * 4);
  if (d->n_counts) std::memcpy(table.data() + xy_bytes + rec_bytes + len_bytes, d->counts, (size_t)d->n_counts * 4);
  // pageable host memory: the copy has left `table` when the call returns
  hipError_t e = hipMemcpyAsync(d->ws, table.data(), (size_t)need, hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;

  const unsigned char *ws = (const unsigned char *)d->ws;
  CocoParams p;
  p.xy = (const double *)ws;
  p.recs = (const ymi_coco_mask_rec *)(ws + xy_bytes);
  p.poly_len = (const int32_t *)(ws + xy_bytes + rec_bytes);
  p.counts = (const uint32_t *)(ws + xy_bytes + rec_bytes + len_bytes);
  p.n = d->n;
  const int64_t words = (max_pixels + 32) / 32;
  if (words <= kW0) launch<kW0>(p, (hipStream_t)stream);
  else if (words <= kW1) launch<kW1>(p, (hipStream_t)stream);
  else if (words <= kW2) launch<kW2>(p, (hipStream_t)stream);
  else launch<kW3>(p, (hipStream_t)stream);
  return ymi_launch_status();
}
