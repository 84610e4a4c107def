// Scaffolding shared by the fp16x2 convolution kernels (fp32 operands carried as two fp16 planes on the fp16 MFMAs): conv_igemm.hip,
// dcn.hip, pcconv.hip, wstat.hip, patch.hip, patch2.hip, chain.hip, chain2.hip, wgemm.hip.  One definition of the buffer-resource
// word, the plane split, the counted wait / barrier pair, the activation slope and the residency cap of the
// launchers.  The short names live in namespace ymi_h2, which the files' anonymous namespaces pull in.
#pragma once
#include "common.h"
#include "../../include/yolact_amd.h"

// counted wait for the oldest vector-memory operations (vmcnt is in order) / LDS traffic drained + one raw s_barrier
#define YMI_WAIT_VM(N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory")
#define YMI_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// none / ReLU / LeakyReLU(0.1) as  v = max(v, slope * v)
__device__ __forceinline__ float ymi_act_slope(int act) { return act == YMI_ACT_RELU ? 0.f : (act == YMI_ACT_LEAKY01 ? 0.1f : 1.f); }

namespace ymi_h2 {

constexpr int BK = 32;                  // K chunk
constexpr unsigned OOB = 0x80000000u;   // buffer offset >= num_records (< 2^31, validated): the load returns zeros, a store is dropped

typedef __attribute__((address_space(3))) void *lds_ptr_t;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// raw buffer resource over `bytes` bytes at p (offsets past it: see OOB)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void *p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, bytes, 0x00020000);
}

// ---- fp32-class products on the fp16 matrix pipe ("fp16x2") ---------------------------------------------------------------
// x * s = h + l, two fp16 pieces by ROUND TO NEAREST (v_cvt_pk_f16_f32): h = fp16(x s), l = fp16(x s - h) with x s - h exact
// in fp32.  11 + 11 significant bits + two signs represent about two thirds of all fp32 values exactly and the rest to one fp32 ulp,
// unbiased.  s = a power of two per tensor (ymi_h2_scale: the producer's magnitude bound -> [2^13, 2^14)), so h never
// overflows and stays a normal fp16 for 27 binades below the tensor's maximum.  a*b = hh + hl + lh (+ ll dropped,
// <= 2^-22 |ab|): 3 MFMAs (v_mfma_f32_32x32x16_f16, exact products, fp32 accumulate) instead of bf16x3's 6, and the split
// is 3 VALU per element with no byte permutes.  tools/split_probe.hip: 574 TFLOP/s fp32-equivalent on random data (bf16x3
// 313, exact fp32 154), error against fp64 2.6e-7 of sum|ab| (bf16x3 3.3e-7, fp32 MFMA 5.2e-7).
struct Split2 { f16x8 h, l; };
using Frag = Split2;

__device__ __forceinline__ Split2 split8h(const f32x4 x0, const f32x4 x1, const float s) {
  const float x[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
  Split2 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float t = x[e] * s;
    const _Float16 h = (_Float16)t;
    o.h[e] = h;
    o.l[e] = (_Float16)(t - (float)h);
  }
  return o;
}
// four values -> elements o .. o + 3 of the two planes (f16x4, or one half of an f16x8 fragment)
template <class V>
__device__ __forceinline__ void split4h(const f32x4 x, const float s, V &h, V &l, int o = 0) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float t = x[e] * s;
    const _Float16 hi = (_Float16)t;
    h[o + e] = hi;
    l[o + e] = (_Float16)(t - (float)hi);
  }
}

#ifdef YMI_DIAGNOSTICS
// words 10 .. 15 of a block's 16-word trace record (tools/pipe_trace.py): real-time clock at start / now, where the wave ran, chunks
__device__ __forceinline__ void trace_tail(unsigned long long *o, unsigned long long rt0, int nk) {
  o[10] = rt0;
  o[11] = __builtin_amdgcn_s_memrealtime();
  o[12] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);                                   // HW_REG_HW_ID
  o[13] = (unsigned long long)(__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7u);                            // XCC_ID
  o[14] = (unsigned long long)nk;
  o[15] = 1;
}
#endif

// ---- host side: residency cap ------------------------------------------------------------------------------------------------
// The workgroup dispatcher does not balance a grid that fits in one residency round: it packs up to `occupancy`
// blocks on a CU while others hold fewer (a 616-block layer ran as if its busiest CU held 4+ blocks, not 3).  When
// the grid is at most occ*256 blocks we therefore cap residency at k = ceil(grid / 256) blocks per CU by padding
// the block's LDS allocation with unused dynamic LDS, so no CU can take more than its share.
// Returns the dynamic LDS bytes to launch with (0: no cap) for a kernel of `static_lds` bytes that runs `occ` blocks per CU.
constexpr int LDS_PER_CU = 160 * 1024, NUM_CU = 256;
static inline int residency_cap_lds(int static_lds, int occ, int blocks) {
  const int k = (blocks + NUM_CU - 1) / NUM_CU;           // blocks per CU if perfectly spread
  if (k < occ) {
    const int want = LDS_PER_CU / (k + 1) + 1024;         // > 160K/(k+1)  =>  at most k blocks fit
    if (want > static_lds && want <= LDS_PER_CU / k) return want - static_lds;
  }
  return 0;
}

}  // namespace ymi_h2
