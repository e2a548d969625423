// Body of pe_inputs_kernel / pe_inputs_ld_kernel (geometry.hip includes it once per kernel, so that the kernel without a pitch keeps its instruction
// stream).  MV2D_FR_LD: the row pitch of A_frustum and A_frustum_f32 -- (3 * D), or the argument ld (a multiple of 8); MV2D_FR_PITCHED: 1 = their
// columns 3 D .. ld - 1 are written as zeros.
    __shared__ __attribute__((aligned(16))) unsigned short rowbuf[4][3 * 256 + 384];      // frustum row (<= 768 values) | sine row (384)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x * 4 + wave;
    if (s >= *S_dev) return;                                  // (whole waves leave; no block barrier below)
    // (the position is the same for all lanes of the wave: made uniform explicitly, so that the per-view matrix and the column / row
    // coordinates are scalar loads instead of 14 broadcast vector loads per lane)
    const int pos = __builtin_amdgcn_readfirstlane(s2pos[s]);
    const int v = pos / (h * w), rem = pos - v * h * w, y = rem / w, x = rem - y * w;
    unsigned short* fr_row = rowbuf[wave];
    unsigned short* si_row = rowbuf[wave] + 3 * 256;
    // feature row gather (fp32 kept for the K = feat + pe sum, key16 for the SE gate and the value rows)
    {
        const float4 f = MapElem<MT>::widen(MapElem<MT>::ld4(featcl + (long long)pos * C + 4 * lane));
        if (Xf_f32) *reinterpret_cast<float4*>(Xf_f32 + (long long)s * C + 4 * lane) = f;
        *reinterpret_cast<uint2*>(Xf_k16 + (long long)s * C + 4 * lane) = make_uint2(pack_k16x2(f.x, f.y), pack_k16x2(f.z, f.w));
    }
    if constexpr (EXACT) {
        for (int dk = lane; dk < D; dk += 64) {
            const double d = coords_d[dk];
            const double dm = d < 1e-3 ? 1e-3 : d;
            const double p[4] = {coords_w[x] * dm, coords_h[y] * dm, d, 1.0};
            const double* M = img2lidar + v * 16;
            const double pr[3] = {pr0, pr1, pr2}, pd[3] = {pd0, pd1, pd2};
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) acc = acc + M[i * 4 + k] * p[k];
                double n = (acc - pr[i]) / pd[i];
                n = n < 0.0 ? 0.0 : (n > 1.0 ? 1.0 : n);          // inverse_sigmoid: clamp(0,1)
                const double x1 = n < 1e-5 ? 1e-5 : n;
                const double x2 = (1.0 - n) < 1e-5 ? 1e-5 : (1.0 - n);
                fr_row[dk * 3 + i] = f32_to_k16(logf((float)x1 / (float)x2));
                // index-exact route: the unrounded fp32 row, every step in fp64 and in the reference's operation order (MU/pe.py:119-130)
                A_frustum_f32[(long long)s * MV2D_FR_LD + dk * 3 + i] = (float)log(x1 / x2);
            }
        }
#if MV2D_FR_PITCHED
        for (int c = 3 * D + lane; c < ld; c += 64) A_frustum_f32[(long long)s * ld + c] = 0.f;
#endif
    } else {
        // default route (round 4): the point of depth bin d is linear in d -- M (cw dm, ch dm, d, 1) = dm (M0 cw + M1 ch) + d M2 + M3 -- so the
        // per-position part is hoisted (wave-uniform) and a coordinate costs two fp64 FMAs; the normalisation multiplies by 1 / range.  (Before:
        // 4 fp64 products + sums and an fp64 DIVISION per coordinate, 192 per position; 96.8 -> 88.6 us per 140 k positions.)  The fp64 result
        // moves by ~1e-16 relative; it is rounded to fp32 for the quotient / logarithm and to key16 right after.
        const double* M = img2lidar + v * 16;
        const double cw = coords_w[x], chh = coords_h[y];
        const double u[3] = {fma(M[0], cw, M[1] * chh), fma(M[4], cw, M[5] * chh), fma(M[8], cw, M[9] * chh)};
        const double m2[3] = {M[2], M[6], M[10]}, m3[3] = {M[3] - pr0, M[7] - pr1, M[11] - pr2};
        const double ipd[3] = {1.0 / pd0, 1.0 / pd1, 1.0 / pd2};
        for (int dk = lane; dk < D; dk += 64) {
            const double d = coords_d[dk];
            const double dm = d < 1e-3 ? 1e-3 : d;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double n = fma(u[i], dm, fma(m2[i], d, m3[i])) * ipd[i];
                n = n < 0.0 ? 0.0 : (n > 1.0 ? 1.0 : n);          // inverse_sigmoid: clamp(0,1)
                const double x1 = n < 1e-5 ? 1e-5 : n;
                const double x2 = (1.0 - n) < 1e-5 ? 1e-5 : (1.0 - n);
                // quotient and logarithm in fp32: 1e-7 absolute against a value that is rounded to key16 (fp16) right here
                fr_row[dk * 3 + i] = f32_to_k16(logf((float)x1 / (float)x2));
            }
        }
    }
    // sine features, channel order (n | y | x).  NOT interleaved: the reference stacks sin/cos on dim=4 of a
    // 5-D tensor (MU/positional_encoding.py:86-94), so within an axis channels 0..63 = sin(e / dim_t[2j]) and
    // channels 64..127 = cos(e / dim_t[2j+1]).
#if MV2D_FR_PITCHED
    for (int c = 3 * D + lane; c < ld; c += 64) fr_row[c] = 0;
#endif
    if (!A_sine) {                                            // the sine branch comes from the engine's folded table: only the frustum row is needed
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);
        const int nf0 = MV2D_FR_LD / 8;
        for (int q = lane; q < nf0; q += 64)
            *reinterpret_cast<uint4*>(A_frustum + (long long)s * MV2D_FR_LD + 8 * q) = *reinterpret_cast<const uint4*>(fr_row + 8 * q);
        return;
    }
    const float en = embeds[pos], ey = embeds[P + pos], ex = embeds[2 * P + pos];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int ch = lane + 64 * k;
        const int axis = ch >> 7, i = ch & 127;
        const float e = axis == 0 ? en : (axis == 1 ? ey : ex);
        // arguments lie in [0, 2 pi]: the hardware sin / cos (v_sin_f32 on x / 2 pi, ~1e-6 absolute) is as good as the library call
        // for a value that is rounded to key16 (fp16) right here
        const float a = e / dim_t[i < 64 ? 2 * i : 2 * (i - 64) + 1];
        si_row[ch] = f32_to_k16(i < 64 ? __sinf(a) : __cosf(a));
        if (EXACT) A_sine_f32[(long long)s * 384 + ch] = i < 64 ? sinf(a) : cosf(a);
    }
    __builtin_amdgcn_wave_barrier();                          // the rows are read back by the same wave only
    __builtin_amdgcn_s_waitcnt(0xc07f);                       // lgkmcnt(0): LDS writes landed
    const int nf = MV2D_FR_LD / 8;                                 // 16-byte chunks of the frustum row (D % 8 == 0)
    for (int q = lane; q < nf; q += 64)
        *reinterpret_cast<uint4*>(A_frustum + (long long)s * MV2D_FR_LD + 8 * q) = *reinterpret_cast<const uint4*>(fr_row + 8 * q);
    if (lane < 48) *reinterpret_cast<uint4*>(A_sine + (long long)s * 384 + 8 * lane) = *reinterpret_cast<const uint4*>(si_row + 8 * lane);
