// The split-precision PE block (pe_x3_kernel.h): its 64-bin instance pe_x3_kernel<MT> and the C entries.
#include "pe_x3_kernel.h"

#ifdef MV2D_PX_TRACE
extern "C" int mv2d_px_trace_read(long long* host, int n) { return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_px_trace), n * sizeof(long long)) == hipSuccess ? 0 : -2; }
#endif

// C-ABI: include/mv2d_hip.h
template <class MT>
static void pe_x3_launch(const float* A1, const void* Xmap, const int* row_index, const int* m_dev, int M,
                         const void* W1a_hi, const void* W1a_lo, const float* b1a, const void* W1b_hi, const void* W1b_lo, const float* b1b,
                         const void* Wr_hi, const void* Wr_lo, const float* br, const void* We_hi, const void* We_lo, const float* be,
                         const float* sine_tab, int tab_period, float* pe, void* Xk_hi, void* Xk_lo, void* Xv_hi, void* Xv_lo, int lo_fmt, int pe_at_index, int* lo8_flag, int Kp, void* stream) {
    PeX3ParamsT<MT> p{A1, (const MT*)Xmap, row_index, m_dev, M, (const unsigned short*)W1a_hi, (const unsigned short*)W1a_lo, b1a, (const unsigned short*)W1b_hi,
                      (const unsigned short*)W1b_lo, b1b, (const unsigned short*)Wr_hi, (const unsigned short*)Wr_lo, br, (const unsigned short*)We_hi,
                      (const unsigned short*)We_lo, be, sine_tab, tab_period, pe, (unsigned short*)Xk_hi, (unsigned short*)Xk_lo, (unsigned short*)Xv_hi,
                      (unsigned short*)Xv_lo, lo_fmt, lo8_flag, pe_at_index};
    const int ks1 = Kp / 32, blocks = cdiv(M, BM);
    if (ks1 == 6) hipLaunchKernelGGL(pe_x3_kernel<MT>, dim3(blocks), dim3(NTHR), 0, (hipStream_t)stream, p);
    else if (!mv2d_px_launch_d1<MT>(p, ks1, blocks, (hipStream_t)stream)) mv2d_px_launch_d2<MT>(p, ks1, blocks, (hipStream_t)stream);     // (the entry checked Kp)
}

// map_fmt: element format of the feature map Xmap (common.h: 0 = fp32, 1 = fp16, 2 = bf16)
// Kp: columns (= row pitch) of A1 and K of W1a, 3 * depth_num zero-padded to a multiple of 32 (32 .. 256; 192 = the 64 bins of mv2d_pe_fused_x3_fmt)
extern "C" int mv2d_pe_fused_x3_k(const float* A1, const void* Xmap, const int* row_index, const int* m_dev, int M,
                                    const void* W1a_hi, const void* W1a_lo, const float* b1a, const void* W1b_hi, const void* W1b_lo, const float* b1b,
                                    const void* Wr_hi, const void* Wr_lo, const float* br, const void* We_hi, const void* We_lo, const float* be,
                                    const float* sine_tab, int tab_period, float* pe, void* Xk_hi, void* Xk_lo, void* Xv_hi, void* Xv_lo, int lo_fmt, int pe_at_index, int* lo8_flag,
                                    int map_fmt, int Kp, void* stream) {
    MV2D_CHECK_ARG(Kp >= 32 && Kp <= 256 && Kp % 32 == 0, "mv2d_pe_fused_x3_k: Kp (32 * ceil(3 * depth_num / 32)) must be a multiple of 32 in [32, 256]");
    MV2D_CHECK_ARG(A1 && Xmap && W1a_hi && W1a_lo && b1a && W1b_hi && W1b_lo && b1b && Wr_hi && Wr_lo && br && We_hi && We_lo && be && sine_tab,
                   "mv2d_pe_fused_x3: null pointer");
    MV2D_CHECK_ARG(pe || Xk_hi, "mv2d_pe_fused_x3: no output");
    MV2D_CHECK_ARG(!pe_at_index || (pe && row_index), "mv2d_pe_fused_x3: pe_at_index needs pe and row_index");
    MV2D_CHECK_ARG((Xk_hi != nullptr) == (Xk_lo != nullptr) && (Xk_hi != nullptr) == (Xv_hi != nullptr) && (Xk_hi != nullptr) == (Xv_lo != nullptr),
                   "mv2d_pe_fused_x3: the four key / value row outputs come together");
    MV2D_CHECK_ARG(M >= 0 && tab_period > 0, "mv2d_pe_fused_x3: M must be >= 0 and tab_period > 0");
    MV2D_CHECK_ARG(lo_fmt == 0 || lo_fmt == 1, "mv2d_pe_fused_x3: lo_fmt is 0 (key16 lo rows) or 1 (e4m3 lo rows)");
    MV2D_CHECK_ARG(map_fmt >= 0 && map_fmt <= 2, "mv2d_pe_fused_x3_fmt: map_fmt is 0 (fp32), 1 (fp16) or 2 (bf16)");
    MV2D_CHECK_ARG(((uintptr_t)A1 & 15) == 0 && ((uintptr_t)Xmap & (map_fmt ? 7 : 15)) == 0 && ((uintptr_t)sine_tab & 15) == 0,
                   "mv2d_pe_fused_x3: rows must be 16-byte aligned (a 16-bit map: 8-byte)");
    if (M == 0) return MV2D_OK;
    MV2D_MAP_DISPATCH(map_fmt, pe_x3_launch<MT>(A1, Xmap, row_index, m_dev, M, W1a_hi, W1a_lo, b1a, W1b_hi, W1b_lo, b1b, Wr_hi, Wr_lo, br, We_hi, We_lo, be, sine_tab,
                                                tab_period, pe, Xk_hi, Xk_lo, Xv_hi, Xv_lo, lo_fmt, pe_at_index, lo8_flag, Kp, stream));
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}

// The PE without the feature-guided gate (with_fpe=False): pe_x3_nogate_kernel<MT, Kp / 32>.  No Wr / We / br / be; Xmap may be NULL when no key / value
// rows are asked for (the kernel then reads no feature row).
template <class MT>
static void pe_x3_ng_launch(const float* A1, const void* Xmap, const int* row_index, const int* m_dev, int M,
                            const void* W1a_hi, const void* W1a_lo, const float* b1a, const void* W1b_hi, const void* W1b_lo, const float* b1b,
                            const float* sine_tab, int tab_period, float* pe, void* Xk_hi, void* Xk_lo, void* Xv_hi, void* Xv_lo, int lo_fmt, int pe_at_index, int* lo8_flag, int Kp, void* stream) {
    PeX3ParamsT<MT> p{A1, (const MT*)Xmap, row_index, m_dev, M, (const unsigned short*)W1a_hi, (const unsigned short*)W1a_lo, b1a, (const unsigned short*)W1b_hi,
                      (const unsigned short*)W1b_lo, b1b, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, sine_tab, tab_period, pe, (unsigned short*)Xk_hi,
                      (unsigned short*)Xk_lo, (unsigned short*)Xv_hi, (unsigned short*)Xv_lo, lo_fmt, lo8_flag, pe_at_index};
    const int ks1 = Kp / 32, blocks = cdiv(M, BM);
    if (!mv2d_px_launch_ng1<MT>(p, ks1, blocks, (hipStream_t)stream)) mv2d_px_launch_ng2<MT>(p, ks1, blocks, (hipStream_t)stream);     // (the entry checked Kp)
}

extern "C" int mv2d_pe_fused_x3_ng(const float* A1, const void* Xmap, const int* row_index, const int* m_dev, int M,
                                   const void* W1a_hi, const void* W1a_lo, const float* b1a, const void* W1b_hi, const void* W1b_lo, const float* b1b,
                                   const float* sine_tab, int tab_period, float* pe, void* Xk_hi, void* Xk_lo, void* Xv_hi, void* Xv_lo, int lo_fmt, int pe_at_index, int* lo8_flag,
                                   int map_fmt, int Kp, void* stream) {
    MV2D_CHECK_ARG(Kp >= 32 && Kp <= 256 && Kp % 32 == 0, "mv2d_pe_fused_x3_ng: Kp (32 * ceil(3 * depth_num / 32)) must be a multiple of 32 in [32, 256]");
    MV2D_CHECK_ARG(A1 && W1a_hi && W1a_lo && b1a && W1b_hi && W1b_lo && b1b && sine_tab, "mv2d_pe_fused_x3_ng: null pointer");
    MV2D_CHECK_ARG(pe || Xk_hi, "mv2d_pe_fused_x3_ng: no output");
    MV2D_CHECK_ARG(!pe_at_index || (pe && row_index), "mv2d_pe_fused_x3_ng: pe_at_index needs pe and row_index");
    MV2D_CHECK_ARG((Xk_hi != nullptr) == (Xk_lo != nullptr) && (Xk_hi != nullptr) == (Xv_hi != nullptr) && (Xk_hi != nullptr) == (Xv_lo != nullptr),
                   "mv2d_pe_fused_x3_ng: the four key / value row outputs come together");
    MV2D_CHECK_ARG(Xmap || !Xk_hi, "mv2d_pe_fused_x3_ng: the key / value row outputs need the feature map Xmap");
    MV2D_CHECK_ARG(M >= 0 && tab_period > 0, "mv2d_pe_fused_x3_ng: M must be >= 0 and tab_period > 0");
    MV2D_CHECK_ARG(lo_fmt == 0 || lo_fmt == 1, "mv2d_pe_fused_x3_ng: lo_fmt is 0 (key16 lo rows) or 1 (e4m3 lo rows)");
    MV2D_CHECK_ARG(map_fmt >= 0 && map_fmt <= 2, "mv2d_pe_fused_x3_ng: map_fmt is 0 (fp32), 1 (fp16) or 2 (bf16)");
    MV2D_CHECK_ARG(((uintptr_t)A1 & 15) == 0 && ((uintptr_t)Xmap & (map_fmt ? 7 : 15)) == 0 && ((uintptr_t)sine_tab & 15) == 0,
                   "mv2d_pe_fused_x3_ng: rows must be 16-byte aligned (a 16-bit map: 8-byte)");
    if (M == 0) return MV2D_OK;
    MV2D_MAP_DISPATCH(map_fmt, pe_x3_ng_launch<MT>(A1, Xmap, row_index, m_dev, M, W1a_hi, W1a_lo, b1a, W1b_hi, W1b_lo, b1b, sine_tab, tab_period, pe, Xk_hi, Xk_lo,
                                                   Xv_hi, Xv_lo, lo_fmt, pe_at_index, lo8_flag, Kp, stream));
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}

extern "C" int mv2d_pe_fused_x3_fmt(const float* A1, const void* Xmap, const int* row_index, const int* m_dev, int M,
                                    const void* W1a_hi, const void* W1a_lo, const float* b1a, const void* W1b_hi, const void* W1b_lo, const float* b1b,
                                    const void* Wr_hi, const void* Wr_lo, const float* br, const void* We_hi, const void* We_lo, const float* be,
                                    const float* sine_tab, int tab_period, float* pe, void* Xk_hi, void* Xk_lo, void* Xv_hi, void* Xv_lo, int lo_fmt, int pe_at_index, int* lo8_flag,
                                    int map_fmt, void* stream) {
    return mv2d_pe_fused_x3_k(A1, Xmap, row_index, m_dev, M, W1a_hi, W1a_lo, b1a, W1b_hi, W1b_lo, b1b, Wr_hi, Wr_lo, br, We_hi, We_lo, be, sine_tab, tab_period, pe,
                              Xk_hi, Xk_lo, Xv_hi, Xv_lo, lo_fmt, pe_at_index, lo8_flag, map_fmt, 192, stream);
}

extern "C" int mv2d_pe_fused_x3(const float* A1, const float* Xmap, const int* row_index, const int* m_dev, int M,
                                const void* W1a_hi, const void* W1a_lo, const float* b1a, const void* W1b_hi, const void* W1b_lo, const float* b1b,
                                const void* Wr_hi, const void* Wr_lo, const float* br, const void* We_hi, const void* We_lo, const float* be,
                                const float* sine_tab, int tab_period, float* pe, void* Xk_hi, void* Xk_lo, void* Xv_hi, void* Xv_lo, int lo_fmt, int pe_at_index, int* lo8_flag, void* stream) {
    return mv2d_pe_fused_x3_fmt(A1, Xmap, row_index, m_dev, M, W1a_hi, W1a_lo, b1a, W1b_hi, W1b_lo, b1b, Wr_hi, Wr_lo, br, We_hi, We_lo, be, sine_tab, tab_period, pe,
                                Xk_hi, Xk_lo, Xv_hi, Xv_lo, lo_fmt, pe_at_index, lo8_flag, MV2D_MAP_F32, stream);
}
