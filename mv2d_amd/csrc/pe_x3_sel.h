// The VIEW FILTER of the split-precision PE kernels (two-frame head, route option pe_cache_views): a launch takes only the rows of some views of a
// sample, so that the rows of views whose camera matrices repeat run the gate on a cached frustum MLP (pe_x3_gate_rows_kernel, pe_x3_gate.hip) and
// the rows of the other views the full kernel (pe_x3_sel_kernel below), side by side into the same row buffers.
//   row m lies at map position pos = row_index[m] (m without a row_index), in view (pos % tab_period) / hw of its sample (tab_period = views * hw,
//   at most 32 views); view_mask: ONE word in device memory, read by the kernel (a captured graph does not depend on its value); take_set != 0: the
//   launch takes the rows whose view bit is set, take_set == 0: the rows whose bit is clear.
// A block none of whose rows is taken returns before its first barrier (every wave looks at all 64 rows of the tile: a block-uniform answer); a
// mixed tile is computed whole and its stores are masked per row, so any row order is correct and a sorted list (the key list of the T path is sorted
// by position) makes the skip effective.
// pe_x3_sel_kernel<MT, KS1> is pe_x3_body.inc once more with the two hooks filled in: the schedule, the arithmetic and every written row are those of
// pe_x3_kernel / pe_x3_depth_kernel.  Instances in translation units of their own (pe_x3_sel1.hip: KS1 = 1 .. 4 and the C entry, pe_x3_sel2.hip: 5 .. 8).
#pragma once
#include "pe_x3_kernel.h"

struct PeViewSel { const unsigned* view_mask; int hw; int take_set; };

template <class MT>
struct PeX3SelParamsT { PeX3ParamsT<MT> p; PeViewSel sel; };

template <class MT> bool mv2d_px_launch_sel1(const PeX3SelParamsT<MT>& q, int ks1, int blocks, hipStream_t stream);
template <class MT> bool mv2d_px_launch_sel2(const PeX3SelParamsT<MT>& q, int ks1, int blocks, hipStream_t stream);

// the argument checks the entries with a view filter share (`who`: the entry's name)
#define MV2D_CHECK_VIEW_SEL(who, view_mask, hw, tab_period)                                                                                   \
    MV2D_CHECK_ARG((view_mask) && (hw) > 0 && (tab_period) > 0 && (tab_period) % (hw) == 0 && (tab_period) / (hw) <= 32,                      \
                   who ": the view filter needs view_mask (one device word), hw > 0, tab_period % hw == 0 and at most 32 views (tab_period / hw)")

namespace {

static_assert(BM == 64, "sel_tile_any: one lane per row of the tile");

__device__ __forceinline__ bool sel_take(unsigned mask, int pos, int tab_period, const PeViewSel& s) {
    return (((mask >> ((pos % tab_period) / s.hw)) & 1u) != 0u) == (s.take_set != 0);
}

// does the tile m0 .. m0 + 63 hold a row this launch takes?  Asked by every wave for all rows of the tile (lane = row): block-uniform without a barrier
__device__ __forceinline__ bool sel_tile_any(unsigned mask, const int* __restrict__ row_index, int m0, int M, int lane, int tab_period, const PeViewSel& s) {
    const int m = m0 + lane;
    bool t = false;
    if (m < M) t = sel_take(mask, row_index ? row_index[m] : m, tab_period, s);
    return __builtin_amdgcn_ballot_w64(t) != 0;
}

// bit k: row ri[k] of the output phase's read-back mapping is taken
template <int NK>
__device__ __forceinline__ unsigned sel_rows(unsigned mask, const int (&ri)[NK], int tab_period, const PeViewSel& s) {
    unsigned taken = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) taken |= (sel_take(mask, ri[k], tab_period, s) ? 1u : 0u) << k;
    return taken;
}

#undef PX_SEL_BLOCK
#undef PX_SEL_ROWS
#undef PX_SEL_TAKEN
#define PX_SEL_BLOCK()                                                                                      \
    const unsigned sel_mask = *q.sel.view_mask;                                                             \
    if (!sel_tile_any(sel_mask, p.row_index, m0, M, lane, p.tab_period, q.sel)) return
#define PX_SEL_ROWS() const unsigned sel_taken = sel_rows(sel_mask, ri, p.tab_period, q.sel)
#define PX_SEL_TAKEN(k) ((sel_taken >> (k)) & 1u)

template <class MT, int KS1>
__global__ __launch_bounds__(NTHR, 1) void pe_x3_sel_kernel(PeX3SelParamsT<MT> q) {
    using S = Sched<KS1>;
    const PeX3ParamsT<MT>& p = q.p;
#include "pe_x3_body.inc"
}

#undef PX_SEL_BLOCK
#undef PX_SEL_ROWS
#undef PX_SEL_TAKEN

}  // namespace
