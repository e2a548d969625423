// The GATE of the split-precision PE block alone (pe_x3_kernel.h, from "---- 2. the gate" onward) on a cached frustum MLP:
//   G  = sigmoid(conv_expand(relu(conv_reduce(feat))))          256 -> 256 -> 256      (MU/pe.py:36-48, 162-166)
//   pe = tab[position] + Q[position] * G                         Q = position_encoder(A1) + b1b, constant per (weights, padding geometry, camera matrices)
// Q is what the gate-less kernel (pe_x3_nogate_kernel on a zero table) writes for all positions of one sample: the rounded P1 + b1b of the gated
// kernel bit for bit, so pe is bit for bit the gated kernel's (the product and the table sum stay two roundings: gate_out below).  The 16 k-steps
// of part 4 of the gated schedule run on the same ring, the same LDS images and in the same MFMA order; parts 0..3 (56 of 72 k-steps at 64 bins), the
// frustum rows and the W1a / W1b streams are gone.  The feature tile is requested first thing in the block (nothing to hide it under any more), the Q and
// table rows of an output half where the gated kernel requests its table rows.  One instance per map format; no depth instances (the depth only
// shapes Q); pe output only (the S path reads nothing else).
// pe_x3_gate_rows_kernel (T path, route option pe_cache_views) is the same body with the output phase of pe_x3_body.inc -- Xk = split(pe + feat), Xv =
// split(feat) as key16 hi rows and key16 or e4m3 lo rows, the fp32 feature pieces requested with the table and Q rows -- and the view filter of
// pe_x3_sel.h: it writes the rows of the views whose bit is set, bit for bit the rows of pe_x3_kernel, and leaves the others to pe_x3_sel_kernel.
#include "pe_x3_sel.h"

template <class MT>
struct PeGateParamsT {
    const float* Q; const MT* Xmap; const int* row_index; const int* m_dev; int M;
    const unsigned short* Wr_h; const unsigned short* Wr_l; const float* br; const unsigned short* We_h; const unsigned short* We_l; const float* be;
    const float* sine_tab; int tab_period;
    float* pe; int pe_at_index;
};

// the row outputs and the view filter of pe_x3_gate_rows_kernel (PeX3ParamsT's fields of the same names; pe_x3_sel.h)
struct PeGateRows {
    unsigned short* Xk_hi; unsigned short* Xk_lo; unsigned short* Xv_hi; unsigned short* Xv_lo; int lo8; int* lo8_flag;
    PeViewSel sel;
};

namespace {

enum { G_R = 0, G_E = 256, G_FLOATS = 512 };
constexpr int SMEM_G = 4 * IMG + G_FLOATS * 4;

// tab + q * g in TWO roundings (the gated kernel rounds (P1 + b) * g on its way through LDS, then adds the table row): no contraction to an FMA
__device__ __forceinline__ float4 gate_out(const float4& tv, const float4& q, const float4& g) {
#pragma clang fp contract(off)
    const float4 pr = make_float4(q.x * g.x, q.y * g.y, q.z * g.z, q.w * g.w);
    return make_float4(pr.x + tv.x, pr.y + tv.y, pr.z + tv.z, pr.w + tv.w);
}

}  // namespace

template <class MT>
__global__ __launch_bounds__(NTHR, 1) void pe_x3_gate_kernel(PeGateParamsT<MT> p) {
#define PX_GATE_ROWS 0
#include "pe_x3_gate_body.inc"
#undef PX_GATE_ROWS
}

template <class MT>
__global__ __launch_bounds__(NTHR, 1) void pe_x3_gate_rows_kernel(PeGateParamsT<MT> p, PeGateRows r) {
#define PX_GATE_ROWS 1
#include "pe_x3_gate_body.inc"
#undef PX_GATE_ROWS
}

// C-ABI: include/mv2d_hip.h
template <class MT>
static void pe_gate_launch(const float* Q, const void* Xmap, const int* row_index, const int* m_dev, int M, const void* Wr_hi, const void* Wr_lo, const float* br,
                           const void* We_hi, const void* We_lo, const float* be, const float* sine_tab, int tab_period, float* pe, int pe_at_index, void* stream) {
    PeGateParamsT<MT> p{Q, (const MT*)Xmap, row_index, m_dev, M, (const unsigned short*)Wr_hi, (const unsigned short*)Wr_lo, br, (const unsigned short*)We_hi,
                        (const unsigned short*)We_lo, be, sine_tab, tab_period, pe, pe_at_index};
    hipLaunchKernelGGL(pe_x3_gate_kernel<MT>, dim3(cdiv(M, BM)), dim3(NTHR), 0, (hipStream_t)stream, p);
}

extern "C" int mv2d_pe_gate_x3(const float* Q, const void* Xmap, const int* row_index, const int* m_dev, int M,
                               const void* Wr_hi, const void* Wr_lo, const float* br, const void* We_hi, const void* We_lo, const float* be,
                               const float* sine_tab, int tab_period, float* pe, void* Xk_hi, void* Xk_lo, void* Xv_hi, void* Xv_lo, int pe_at_index,
                               int map_fmt, void* stream) {
    MV2D_CHECK_ARG(!Xk_hi && !Xk_lo && !Xv_hi && !Xv_lo, "mv2d_pe_gate_x3: no key / value row outputs (pe only: run mv2d_pe_fused_x3_k for the rows)");
    MV2D_CHECK_ARG(Q && Xmap && Wr_hi && Wr_lo && br && We_hi && We_lo && be && sine_tab && pe, "mv2d_pe_gate_x3: null pointer");
    MV2D_CHECK_ARG(!pe_at_index || row_index, "mv2d_pe_gate_x3: pe_at_index needs row_index");
    MV2D_CHECK_ARG(M >= 0 && tab_period > 0, "mv2d_pe_gate_x3: M must be >= 0 and tab_period > 0");
    MV2D_CHECK_ARG(map_fmt >= 0 && map_fmt <= 2, "mv2d_pe_gate_x3: map_fmt is 0 (fp32), 1 (fp16) or 2 (bf16)");
    MV2D_CHECK_ARG(((uintptr_t)Q & 15) == 0 && ((uintptr_t)Xmap & (map_fmt ? 7 : 15)) == 0 && ((uintptr_t)sine_tab & 15) == 0 && ((uintptr_t)pe & 15) == 0,
                   "mv2d_pe_gate_x3: rows must be 16-byte aligned (a 16-bit map: 8-byte)");
    if (M == 0) return MV2D_OK;
    MV2D_MAP_DISPATCH(map_fmt, pe_gate_launch<MT>(Q, Xmap, row_index, m_dev, M, Wr_hi, Wr_lo, br, We_hi, We_lo, be, sine_tab, tab_period, pe, pe_at_index, stream));
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}

template <class MT>
static void pe_gate_rows_launch(const float* Q, const void* Xmap, const int* row_index, const int* m_dev, int M, const void* Wr_hi, const void* Wr_lo, const float* br,
                                const void* We_hi, const void* We_lo, const float* be, const float* sine_tab, int tab_period, float* pe, const PeGateRows& r,
                                void* stream) {
    PeGateParamsT<MT> p{Q, (const MT*)Xmap, row_index, m_dev, M, (const unsigned short*)Wr_hi, (const unsigned short*)Wr_lo, br, (const unsigned short*)We_hi,
                        (const unsigned short*)We_lo, be, sine_tab, tab_period, pe, 0};
    hipLaunchKernelGGL(pe_x3_gate_rows_kernel<MT>, dim3(cdiv(M, BM)), dim3(NTHR), 0, (hipStream_t)stream, p, r);
}

extern "C" int mv2d_pe_gate_rows_x3(const float* Q, const void* Xmap, const int* row_index, const int* m_dev, int M,
                                    const void* Wr_hi, const void* Wr_lo, const float* br, const void* We_hi, const void* We_lo, const float* be,
                                    const float* sine_tab, int tab_period, float* pe, void* Xk_hi, void* Xk_lo, void* Xv_hi, void* Xv_lo, int lo_fmt, int* lo8_flag,
                                    int map_fmt, const unsigned* view_mask, int hw, int take_set, void* stream) {
    MV2D_CHECK_ARG(Q && Xmap && Wr_hi && Wr_lo && br && We_hi && We_lo && be && sine_tab, "mv2d_pe_gate_rows_x3: null pointer");
    MV2D_CHECK_ARG(Xk_hi && Xk_lo && Xv_hi && Xv_lo, "mv2d_pe_gate_rows_x3: the four key / value row outputs are required (pe is optional)");
    MV2D_CHECK_ARG(M >= 0, "mv2d_pe_gate_rows_x3: M must be >= 0");
    MV2D_CHECK_VIEW_SEL("mv2d_pe_gate_rows_x3", view_mask, hw, tab_period);
    MV2D_CHECK_ARG(lo_fmt == 0 || lo_fmt == 1, "mv2d_pe_gate_rows_x3: lo_fmt is 0 (key16 lo rows) or 1 (e4m3 lo rows)");
    MV2D_CHECK_ARG(map_fmt >= 0 && map_fmt <= 2, "mv2d_pe_gate_rows_x3: map_fmt is 0 (fp32), 1 (fp16) or 2 (bf16)");
    MV2D_CHECK_ARG(((uintptr_t)Q & 15) == 0 && ((uintptr_t)Xmap & (map_fmt ? 7 : 15)) == 0 && ((uintptr_t)sine_tab & 15) == 0 && ((uintptr_t)pe & 15) == 0,
                   "mv2d_pe_gate_rows_x3: rows must be 16-byte aligned (a 16-bit map: 8-byte)");
    if (M == 0) return MV2D_OK;
    const PeGateRows r{(unsigned short*)Xk_hi, (unsigned short*)Xk_lo, (unsigned short*)Xv_hi, (unsigned short*)Xv_lo, lo_fmt, lo8_flag, {view_mask, hw, take_set}};
    MV2D_MAP_DISPATCH(map_fmt, pe_gate_rows_launch<MT>(Q, Xmap, row_index, m_dev, M, Wr_hi, Wr_lo, br, We_hi, We_lo, be, sine_tab, tab_period, pe, r, stream));
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}
