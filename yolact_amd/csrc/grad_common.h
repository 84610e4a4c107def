// Shared by the train-mode gradient kernels on the exact-fp32 matrix instruction v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate):
// conv_train.hip (wgrad_k), stem_train.hip (stem_wgrad_k), darknet_train.hip (preconv_wgrad_k), dcn_bwd.hip, and by reference
// conv_dgrad.hip.
//
// STRUCTURE of a weight gradient dw[k,co] = sum_pos a[pos,k] g[pos,co].  The POSITIONS are the instruction's k index, so both operands
// are read in their natural NHWC layout: lane & 31 = the row (of a) or column (of g), the two halves of a wave = two consecutive
// positions.  A lane therefore owns the positions pos0 + half, + 2, + 4, .. of its block's chunk and carries their pixel coordinates
// along (ymi_pos_walk).  The positions are cut into chunks by a rule that reads the shape only (ymi_chunk_plan); a block owns one
// chunk and writes its partial sum to the workspace, [nchunks][rows][Cout]; a second launch adds the partials of every element in chunk
// order from +0.0 (loss_common.h ymi_chunk_sum).  No atomics: the same inputs give the same bits (dcn_bwd.hip alone adds with atomics).
//
// What deliberately stays where it is:
//   wgrad_k's walk (conv_train.hip)  ymi_pos_walk's statements, written out.  Through the struct (the image index a template switch)
//                                wgrad_k<1, 1> got 30 instructions longer and slower: 3x3, 256 -> 96 at 8 x 69 x 69 in 717.9 us, not
//                                691.6 us (+- 2.5); the other five instantiations kept their time (profiles/grad_common_ab.txt).
//   bn_col_sum (bn_train.hip)    lane-strided partials, then the wave butterfly: another order of additions, so another contract.
//   dw_plan (maskiou_loss.hip)   another rule: at least 128 positions per chunk, floor division, chunks of a multiple of 16.
//   crow (stem.hip)              the inference path; the benchmark's kernels are not recompiled for a tidier gradient path.
//   the issue / consume drivers  three lines per kernel around different Grp structs, and dgrad_s2_k's skips its last issue.
#pragma once
#include "loss_common.h"

// row of a 32 x 32 accumulator held in register r by this lane (column = lane & 31, half = lane >> 5)
__device__ __forceinline__ int ymi_acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// A lane's walk over the positions (n, oy, ox) of a [B, H, W] map, two at a time
struct ymi_pos_walk {
  long pos;
  int ox, oy, n;
  __device__ __forceinline__ ymi_pos_walk(long pos_, int W, int H)
      : pos(pos_), ox((int)(pos_ % W)), oy((int)((pos_ / W) % H)), n((int)(pos_ / ((long)W * H))) {}
  __device__ __forceinline__ void step2(const int &W, const int &H) {      // (by value the callers' mask code came out longer)
    pos += 2; ox += 2;
    if (ox >= W) { ox -= W; ++oy; }                      // twice: W (and H) may be 1
    if (ox >= W) { ox -= W; ++oy; }
    if (oy >= H) { oy -= H; ++n; }
    if (oy >= H) { oy -= H; ++n; }
  }
};

// ---- host ------------------------------------------------------------------------------------------------------------------
// P positions in chunks of a multiple of 32: about target_blocks blocks in all when other_blocks blocks work on every chunk
struct ymi_chunks { long per; int nchunks; };
static inline ymi_chunks ymi_chunk_plan(long P, long target_blocks, long other_blocks) {
  const long mb = (P + 31) / 32;
  long sp = (target_blocks + other_blocks - 1) / other_blocks;
  sp = sp < 1 ? 1 : (sp > mb ? mb : sp);
  const long per = (mb + sp - 1) / sp * 32;
  return {per, (int)((P + per - 1) / per)};
}

// nt 32-channel tiles of Cout per wave (a block of four waves covers nt * 128 output channels), gz such blocks
struct ymi_wgrad_tiles { int nt, gz; };
static inline ymi_wgrad_tiles ymi_wgrad_nt(int Cout) {
  const int tiles = (Cout + 31) / 32;
  const int nt = tiles <= 4 ? 1 : (tiles <= 8 ? 2 : 4);
  return {nt, (Cout + nt * 128 - 1) / (nt * 128)};
}
