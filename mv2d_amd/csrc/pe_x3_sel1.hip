// pe_x3_sel_kernel<MT, KS1> (pe_x3_sel.h) for KS1 = 1, 2, 3, 4, and the C entry of the fused split-precision PE block with the view filter.
#include "pe_x3_sel.h"

template <class MT>
bool mv2d_px_launch_sel1(const PeX3SelParamsT<MT>& q, int ks1, int blocks, hipStream_t stream) {
    switch (ks1) {
#define MV2D_PX_SEL(KS1) case KS1: hipLaunchKernelGGL((pe_x3_sel_kernel<MT, KS1>), dim3(blocks), dim3(PX_NTHR), 0, stream, q); return true
        MV2D_PX_SEL(1); MV2D_PX_SEL(2); MV2D_PX_SEL(3); MV2D_PX_SEL(4);
#undef MV2D_PX_SEL
    }
    return false;
}
template bool mv2d_px_launch_sel1<float>(const PeX3SelParamsT<float>&, int, int, hipStream_t);
template bool mv2d_px_launch_sel1<map_f16>(const PeX3SelParamsT<map_f16>&, int, int, hipStream_t);
template bool mv2d_px_launch_sel1<map_bf16>(const PeX3SelParamsT<map_bf16>&, int, int, hipStream_t);

// C-ABI: include/mv2d_hip.h
template <class MT>
static void pe_x3_sel_launch(const float* A1, const void* Xmap, const int* row_index, const int* m_dev, int M,
                             const void* W1a_hi, const void* W1a_lo, const float* b1a, const void* W1b_hi, const void* W1b_lo, const float* b1b,
                             const void* Wr_hi, const void* Wr_lo, const float* br, const void* We_hi, const void* We_lo, const float* be,
                             const float* sine_tab, int tab_period, float* pe, void* Xk_hi, void* Xk_lo, void* Xv_hi, void* Xv_lo, int lo_fmt, int* lo8_flag, int Kp,
                             const unsigned* view_mask, int hw, int take_set, void* stream) {
    PeX3SelParamsT<MT> q{{A1, (const MT*)Xmap, row_index, m_dev, M, (const unsigned short*)W1a_hi, (const unsigned short*)W1a_lo, b1a, (const unsigned short*)W1b_hi,
                          (const unsigned short*)W1b_lo, b1b, (const unsigned short*)Wr_hi, (const unsigned short*)Wr_lo, br, (const unsigned short*)We_hi,
                          (const unsigned short*)We_lo, be, sine_tab, tab_period, pe, (unsigned short*)Xk_hi, (unsigned short*)Xk_lo, (unsigned short*)Xv_hi,
                          (unsigned short*)Xv_lo, lo_fmt, lo8_flag, 0},
                         {view_mask, hw, take_set}};
    const int ks1 = Kp / 32, blocks = cdiv(M, BM);
    if (!mv2d_px_launch_sel1<MT>(q, ks1, blocks, (hipStream_t)stream)) mv2d_px_launch_sel2<MT>(q, ks1, blocks, (hipStream_t)stream);     // (the entry checked Kp)
}

extern "C" int mv2d_pe_fused_x3_k_sel(const float* A1, const void* Xmap, const int* row_index, const int* m_dev, int M,
                                      const void* W1a_hi, const void* W1a_lo, const float* b1a, const void* W1b_hi, const void* W1b_lo, const float* b1b,
                                      const void* Wr_hi, const void* Wr_lo, const float* br, const void* We_hi, const void* We_lo, const float* be,
                                      const float* sine_tab, int tab_period, float* pe, void* Xk_hi, void* Xk_lo, void* Xv_hi, void* Xv_lo, int lo_fmt, int* lo8_flag,
                                      int map_fmt, int Kp, const unsigned* view_mask, int hw, int take_set, void* stream) {
    MV2D_CHECK_ARG(Kp >= 32 && Kp <= 256 && Kp % 32 == 0, "mv2d_pe_fused_x3_k_sel: Kp (32 * ceil(3 * depth_num / 32)) must be a multiple of 32 in [32, 256]");
    MV2D_CHECK_ARG(A1 && Xmap && W1a_hi && W1a_lo && b1a && W1b_hi && W1b_lo && b1b && Wr_hi && Wr_lo && br && We_hi && We_lo && be && sine_tab,
                   "mv2d_pe_fused_x3_k_sel: null pointer");
    MV2D_CHECK_ARG(Xk_hi && Xk_lo && Xv_hi && Xv_lo, "mv2d_pe_fused_x3_k_sel: the four key / value row outputs are required (pe is optional)");
    MV2D_CHECK_ARG(M >= 0, "mv2d_pe_fused_x3_k_sel: M must be >= 0");
    MV2D_CHECK_VIEW_SEL("mv2d_pe_fused_x3_k_sel", view_mask, hw, tab_period);
    MV2D_CHECK_ARG(lo_fmt == 0 || lo_fmt == 1, "mv2d_pe_fused_x3_k_sel: lo_fmt is 0 (key16 lo rows) or 1 (e4m3 lo rows)");
    MV2D_CHECK_ARG(map_fmt >= 0 && map_fmt <= 2, "mv2d_pe_fused_x3_k_sel: map_fmt is 0 (fp32), 1 (fp16) or 2 (bf16)");
    MV2D_CHECK_ARG(((uintptr_t)A1 & 15) == 0 && ((uintptr_t)Xmap & (map_fmt ? 7 : 15)) == 0 && ((uintptr_t)sine_tab & 15) == 0 && ((uintptr_t)pe & 15) == 0,
                   "mv2d_pe_fused_x3_k_sel: rows must be 16-byte aligned (a 16-bit map: 8-byte)");
    if (M == 0) return MV2D_OK;
    MV2D_MAP_DISPATCH(map_fmt, pe_x3_sel_launch<MT>(A1, Xmap, row_index, m_dev, M, W1a_hi, W1a_lo, b1a, W1b_hi, W1b_lo, b1b, Wr_hi, Wr_lo, br, We_hi, We_lo, be, sine_tab,
                                                    tab_period, pe, Xk_hi, Xk_lo, Xv_hi, Xv_lo, lo_fmt, lo8_flag, Kp, view_mask, hw, take_set, stream));
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}
