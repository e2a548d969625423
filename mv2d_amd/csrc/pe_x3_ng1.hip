// pe_x3_nogate_kernel<MT, KS1> (pe_x3_kernel.h) for KS1 = 1, 2, 3, 4: the fused split-precision PE block without the feature-guided gate (with_fpe=False).
#include "pe_x3_kernel.h"

template <class MT>
bool mv2d_px_launch_ng1(const PeX3ParamsT<MT>& p, int ks1, int blocks, hipStream_t stream) {
    switch (ks1) {
#define MV2D_PX_NOGATE(KS1) case KS1: hipLaunchKernelGGL((pe_x3_nogate_kernel<MT, KS1>), dim3(blocks), dim3(PX_NTHR), 0, stream, p); return true
        MV2D_PX_NOGATE(1); MV2D_PX_NOGATE(2); MV2D_PX_NOGATE(3); MV2D_PX_NOGATE(4);
#undef MV2D_PX_NOGATE
    }
    return false;
}
template bool mv2d_px_launch_ng1<float>(const PeX3ParamsT<float>&, int, int, hipStream_t);
template bool mv2d_px_launch_ng1<map_f16>(const PeX3ParamsT<map_f16>&, int, int, hipStream_t);
template bool mv2d_px_launch_ng1<map_bf16>(const PeX3ParamsT<map_bf16>&, int, int, hipStream_t);
