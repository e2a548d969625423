// pe_x3_sel_kernel<MT, KS1> (pe_x3_sel.h) for KS1 = 5, 6, 7, 8: the fused split-precision PE block with the view filter, frustum rows of 32 KS1 columns.
#include "pe_x3_sel.h"

template <class MT>
bool mv2d_px_launch_sel2(const PeX3SelParamsT<MT>& q, int ks1, int blocks, hipStream_t stream) {
    switch (ks1) {
#define MV2D_PX_SEL(KS1) case KS1: hipLaunchKernelGGL((pe_x3_sel_kernel<MT, KS1>), dim3(blocks), dim3(PX_NTHR), 0, stream, q); return true
        MV2D_PX_SEL(5); MV2D_PX_SEL(6); MV2D_PX_SEL(7); MV2D_PX_SEL(8);
#undef MV2D_PX_SEL
    }
    return false;
}
template bool mv2d_px_launch_sel2<float>(const PeX3SelParamsT<float>&, int, int, hipStream_t);
template bool mv2d_px_launch_sel2<map_f16>(const PeX3SelParamsT<map_f16>&, int, int, hipStream_t);
template bool mv2d_px_launch_sel2<map_bf16>(const PeX3SelParamsT<map_bf16>&, int, int, hipStream_t);
