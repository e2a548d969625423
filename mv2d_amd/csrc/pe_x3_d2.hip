// pe_x3_depth_kernel<MT, KS1> (pe_x3_kernel.h) for KS1 = 5, 7, 8: the fused split-precision PE block for frustum rows of 32 KS1 columns.
#include "pe_x3_kernel.h"

template <class MT>
bool mv2d_px_launch_d2(const PeX3ParamsT<MT>& p, int ks1, int blocks, hipStream_t stream) {
    switch (ks1) {
#define MV2D_PX_DEPTH(KS1) case KS1: hipLaunchKernelGGL((pe_x3_depth_kernel<MT, KS1>), dim3(blocks), dim3(PX_NTHR), 0, stream, p); return true
        MV2D_PX_DEPTH(5); MV2D_PX_DEPTH(7); MV2D_PX_DEPTH(8);
#undef MV2D_PX_DEPTH
    }
    return false;
}
template bool mv2d_px_launch_d2<float>(const PeX3ParamsT<float>&, int, int, hipStream_t);
template bool mv2d_px_launch_d2<map_f16>(const PeX3ParamsT<map_f16>&, int, int, hipStream_t);
template bool mv2d_px_launch_d2<map_bf16>(const PeX3ParamsT<map_bf16>&, int, int, hipStream_t);
