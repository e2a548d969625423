// Body of pe_frustum_f32_kernel / pe_frustum_f32_ld_kernel (geometry.hip includes it once per kernel, so that the kernel without a pitch keeps its
// instruction stream).  MV2D_FR_LD: the row pitch of `out` -- (3 * D), or the argument ld; MV2D_FR_PITCHED: 1 = the columns 3 D .. ld - 1 are written as zeros;
// MV2D_FR_SEL: 1 = rows of the views whose bit of *view_mask is set are skipped (view (pos % tab_period) / (h w) of a sample, pe_x3_sel.h).
    __shared__ double tab[256];
    tab[threadIdx.x] = lt.t[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = *S_dev;
    for (int s = blockIdx.x * 4 + wave; s < S; s += gridDim.x * 4) {
        const int pos = __builtin_amdgcn_readfirstlane(s2pos[s]);
#if MV2D_FR_SEL
        if ((*view_mask >> ((pos % tab_period) / (h * w))) & 1u) continue;      // a cached view's row: neither computed nor written (wave-uniform)
#endif
        const int v = pos / (h * w), rem = pos - v * h * w, y = rem / w, x = rem - y * w;
        const double* M = img2lidar + v * 16;
        const double cw = coords_w[x], chh = coords_h[y];
        const double u[3] = {fma(M[0], cw, M[1] * chh), fma(M[4], cw, M[5] * chh), fma(M[8], cw, M[9] * chh)};
        const double m2[3] = {M[2], M[6], M[10]}, m3[3] = {M[3] - pr0, M[7] - pr1, M[11] - pr2};
        const double ipd[3] = {ipd0, ipd1, ipd2};
        for (int dk = lane; dk < D; dk += 64) {
            const double d = coords_d[dk];
            const double dm = d < 1e-3 ? 1e-3 : d;
            float o[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double n = fma(u[i], dm, fma(m2[i], d, m3[i])) * ipd[i];
                n = n < 0.0 ? 0.0 : (n > 1.0 ? 1.0 : n);
                const double x1 = n < 1e-5 ? 1e-5 : n;
                const double x2 = (1.0 - n) < 1e-5 ? 1e-5 : (1.0 - n);
                o[i] = (float)log_diff_tab(x1, x2, tab);
            }
            float* dst = out + (long long)s * MV2D_FR_LD + dk * 3;
            dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
        }
#if MV2D_FR_PITCHED
        for (int c = 3 * D + lane; c < ld; c += 64) out[(long long)s * ld + c] = 0.f;
#endif
    }
