// The chunked window walk of the RoI conv at any RoI size s x s, 1 <= s <= 14: Conv2d(256, 256, 3, padding=1) on the key16 cells of one RoI per block,
// written once (roiconv_walk.inc) for roi_conv_pool_s_kernel (csrc/roiconv.hip: pools the cells) and roi_conv_cells_kernel (csrc/roiconv_cells.hip:
// stores them), which differ only in what they do with a finished chunk.  Also the constants and operand types both files share with the 7 x 7 kernels
// of roiconv.hip.
//
// The walk: the block's RoI (blockIdx.x; a block with roi >= R returns before any barrier) in chunks of 64 output cells (four row tiles,
// ceil(s * s / 64) chunks).  A chunk stages only the cell rows its taps read (its own rows and one above and below: at most 112 cells, s = 14) plus a
// zero row into LDS, then runs the 72 k-steps of the 7 x 7 kernels (weights fragment-major through a 4-deep register ring, a tap is a remapped row
// index, out-of-range neighbours -> the zero row, k order (tap, channel); a rolled loop over the 9 taps, 8 unrolled k-steps each).  At s = 7 the single
// chunk holds the whole RoI.  X3: the split-precision products of roi_conv_pool_x3_kernel (two LDS images, 2 x 60 KB: one block per CU), lo x hi,
// hi x lo, hi x hi into one accumulator; otherwise key16 x key16.  Not tuned: the weights are streamed once per chunk.
// Behind a chunk's MFMAs a lane holds the conv sums of cells c0 + 16 i + 4 fg + r at columns n = 64 wave + 16 j + fr: the walk adds the bias (256 values
// in LDS), applies ReLU and hands every cell below S2 = s * s to the kernel's hook ROI_CONV_WALK_CELL(v, cell, n, j), a statement; roi, S2, wave, fr and
// fg stay declared behind the include.
//
// An .inc body like pe_x3_body.inc with a per-cell hook, not a function template with a per-chunk callable: as the body of a __device__ function, or
// with a lambda that gets the chunk, all four instances came out with other address arithmetic than the spelled-out kernels had (a function's pointer
// parameters are generic, a kernel's are global), the key16 ones with 3 instead of 1 scratch round trips; in this form all four are instruction for
// instruction what they were (profiles/roiconv_walk_kernel_stats.txt).
#pragma once
#include "common.h"

namespace {

constexpr int C = 256;
struct Frag { uint4 u; };                     // one MFMA operand fragment: 8 key16 values (common.h: fp16 since round 4)
typedef unsigned int cv_u32x4 __attribute__((ext_vector_type(4)));
constexpr int GW_ROWS = 120, GW_ZERO = GW_ROWS - 1;     // LDS rows of a window (<= 112 cells) and the index of its zero row

}  // namespace
