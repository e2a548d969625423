// QueryGenerator trunks other than the shipped one (RH/utils/query_generator.py:281-331, 352-363): a shared conv whose cells feed ANOTHER conv or
// the flattened first fc (with_avg_pool=False), and the AvgPool2d(s) of a trunk without convs.
//
// roi_conv_cells_kernel: Conv2d(256, 256, 3, padding=1) + bias + ReLU on the s x s cells of a RoI, 1 <= s <= 14, that WRITES the cells instead of
// pooling them.  The conv is the chunked window walk that roi_conv_pool_s_kernel (csrc/roiconv.hip) runs too: one text, csrc/roiconv_walk.inc
// (described in csrc/roiconv_walk.h), included by both kernels, so the sums of a cell are those the pooled kernel adds up because they are the same
// statements; tests/test_gpu_conv_walk_parent_bits.py holds both to the bytes the two spelled-out copies wrote.  One RoI per block, its cells in chunks
// of 64 output cells; at s = 7 the single chunk holds the whole RoI (the resident shape).
// X3: the cells come as key16 hi + lo pairs, three MFMAs per product (a_lo w_hi + a_hi w_lo + a_hi w_hi); otherwise key16 x key16.
// Outputs (each optional): key16 hi rows [R, s*s, 256] (+ their lo halves: x ~ hi + lo, the split of split_k16x2) for a following conv, fp32 rows
// [R, s*s, 256] = the cell-major flattening the first fc of an un-pooled trunk reads.
// Not tuned: the weights are streamed once per chunk, the epilogue stores 2 / 4 bytes per lane (16 lanes per 32 / 64-byte run).
//
// avgpool_cells_kernel: mean over `cells` consecutive key16 rows (hi, or hi + lo) of 256 channels -> fp32.  cells = s * s: AvgPool2d(s) of the RoI
// cells (num_shared_convs = 0); cells = 1: the fp32 copy of hi + lo rows (the flattened input of a trunk without convs).
#include "roiconv_walk.h"

namespace {

template <bool X3>
__global__ __launch_bounds__(256, X3 ? 1 : 2) void roi_conv_cells_kernel(const unsigned short* __restrict__ feat_hi, const unsigned short* __restrict__ feat_lo,
                                                                        const unsigned short* __restrict__ Wh, const unsigned short* __restrict__ Wl,
                                                                        const float* __restrict__ bias, unsigned short* __restrict__ out_hi,
                                                                        unsigned short* __restrict__ out_lo, float* __restrict__ out_f32, int R, int s) {
// one store per output form
#define ROI_CONV_WALK_CELL(val, cell, n, j)                            \
    do {                                                               \
        const float v = (val);                                         \
        const long long o = ((long long)roi * S2 + (cell)) * C + (n);  \
        if (out_f32) out_f32[o] = v;                                   \
        if (out_hi) {                                                  \
            unsigned int h, l;                                         \
            split_k16x2(v, v, h, l);                                   \
            out_hi[o] = (unsigned short)(h & 0xffffu);                 \
            if (out_lo) out_lo[o] = (unsigned short)(l & 0xffffu);     \
        }                                                              \
    } while (0)
#include "roiconv_walk.inc"
#undef ROI_CONV_WALK_CELL
}

// one block per output row, one channel per thread; four partial sums (cells 4 k + a), added pairwise
__global__ __launch_bounds__(256) void avgpool_cells_kernel(const unsigned short* __restrict__ hi, const unsigned short* __restrict__ lo,
                                                             float* __restrict__ out, int ld_out, int cells) {
    const long long row = blockIdx.x;
    const int n = threadIdx.x;
    const long long base = row * cells * C + n;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < cells; ++c) {
        float v = k16_to_f32(hi[base + (long long)c * C]);
        if (lo) v += k16_to_f32(lo[base + (long long)c * C]);
        a[c & 3] += v;
    }
    out[row * ld_out + n] = ((a[0] + a[1]) + (a[2] + a[3])) / (float)cells;
}

template <bool X3>
int conv_cells(const void* fh, const void* fl, const void* Wh, const void* Wl, const float* bias, void* out_hi, void* out_lo, float* out_f32, int R, int s,
               void* stream) {
    hipLaunchKernelGGL(roi_conv_cells_kernel<X3>, dim3(R), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)fh, (const unsigned short*)fl,
                       (const unsigned short*)Wh, (const unsigned short*)Wl, bias, (unsigned short*)out_hi, (unsigned short*)out_lo, out_f32, R, s);
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}

}  // namespace

// conv3x3 + bias + ReLU on the s x s key16 cells of R RoIs [R, s*s, 256], the cells written: out_hi / out_lo key16 [R, s*s, 256] (out_lo needs out_hi)
// and / or out_f32 [R, s*s, 256]; W = mv2d_pack_wfrag_bf16 of the key16 weight [256, 2304] in k order (tap, channel)
extern "C" int mv2d_qg_conv_cells(const void* roi_feat, const void* W, const float* bias, void* out_hi, void* out_lo, float* out_f32, int R, int roi_size,
                                  void* stream) {
    MV2D_CHECK_ARG(roi_size >= 1 && roi_size <= 14, "mv2d_qg_conv_cells: roi_size must be in [1, 14]");
    MV2D_CHECK_ARG(roi_feat && W && bias && (out_hi || out_f32) && (out_hi || !out_lo) && R >= 0, "mv2d_qg_conv_cells: bad args");
    MV2D_CHECK_ARG(((uintptr_t)roi_feat & 15) == 0 && ((uintptr_t)W & 15) == 0, "mv2d_qg_conv_cells: operands must be 16-byte aligned");
    if (R == 0) return MV2D_OK;
    return conv_cells<false>(roi_feat, nullptr, W, nullptr, bias, out_hi, out_lo, out_f32, R, roi_size, stream);
}

// the same in split precision: cells as key16 hi + lo pairs, W_hi / W_lo = the fragment-major halves of mv2d_split_key16 of the weight
extern "C" int mv2d_qg_conv_cells_x3(const void* roi_feat_hi, const void* roi_feat_lo, const void* W_hi, const void* W_lo, const float* bias, void* out_hi,
                                     void* out_lo, float* out_f32, int R, int roi_size, void* stream) {
    MV2D_CHECK_ARG(roi_size >= 1 && roi_size <= 14, "mv2d_qg_conv_cells_x3: roi_size must be in [1, 14]");
    MV2D_CHECK_ARG(roi_feat_hi && roi_feat_lo && W_hi && W_lo && bias && (out_hi || out_f32) && (out_hi || !out_lo) && R >= 0, "mv2d_qg_conv_cells_x3: bad args");
    MV2D_CHECK_ARG(((uintptr_t)roi_feat_hi & 15) == 0 && ((uintptr_t)roi_feat_lo & 15) == 0 && ((uintptr_t)W_hi & 15) == 0 && ((uintptr_t)W_lo & 15) == 0,
                   "mv2d_qg_conv_cells_x3: operands must be 16-byte aligned");
    if (R == 0) return MV2D_OK;
    return conv_cells<true>(roi_feat_hi, roi_feat_lo, W_hi, W_lo, bias, out_hi, out_lo, out_f32, R, roi_size, stream);
}

// out[r, :] (fp32, row pitch ld_out >= 256) = mean over the `cells` key16 rows r * cells .. of hi (+ lo when given): [R * cells, 256] -> [R, 256]
extern "C" int mv2d_avgpool_cells(const void* hi, const void* lo, float* out, int ld_out, int R, int cells, void* stream) {
    MV2D_CHECK_ARG(hi && out && ld_out >= C && R >= 0 && cells >= 1 && cells <= 196, "mv2d_avgpool_cells: bad args (1 <= cells <= 196, ld_out >= 256)");
    if (R == 0) return MV2D_OK;
    hipLaunchKernelGGL(avgpool_cells_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)hi, (const unsigned short*)lo, out, ld_out,
                       cells);
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}
