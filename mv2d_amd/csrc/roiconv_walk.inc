// The chunked window walk of the RoI conv at any RoI size (csrc/roiconv_walk.h says what it does and who includes it): the text of a kernel body, from
// its first statement to the end of the chunk loop.  The kernel has the parameters feat_hi, feat_lo, Wh, Wl, bias, R, s and the template parameter X3,
// and defines ROI_CONV_WALK_CELL(v, cell, n, j), which gets every cell of a finished chunk.
    constexpr int RING = 4, NIMG = X3 ? 2 : 1;           // ring depth 4 divides the 8 k-steps of a tap: compile-time ring slots in the tap loop
    __shared__ __attribute__((aligned(16))) unsigned char xs[NIMG][GW_ROWS * C * 2];
    __shared__ float bs[C];
    const int roi = blockIdx.x;
    if (roi >= R) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
    const int S2 = s * s;
    const long long w_off = ((long long)(wave * 4) * 64 + lane) * 8;
    constexpr int KS_STRIDE = 16 * 64 * 8, JT_STRIDE = 64 * 8;
    bs[tid] = bias[tid];
    for (int c0 = 0; c0 < S2; c0 += 64) {
        const int last = min(c0 + 63, S2 - 1);
        const int ylo = max(c0 / s - 1, 0), yhi = min(last / s + 1, s - 1);
        const int wb = ylo * s, nwin = (yhi - ylo + 1) * s;          // window: cells [wb, wb + nwin) of the RoI, nwin <= 112
        Frag wqh[RING][4], wql[RING][4];
#pragma unroll
        for (int p = 0; p < RING - 1; ++p)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                wqh[p][j].u = *reinterpret_cast<const uint4*>(Wh + w_off + p * KS_STRIDE + j * JT_STRIDE);
                if (X3) wql[p][j].u = *reinterpret_cast<const uint4*>(Wl + w_off + p * KS_STRIDE + j * JT_STRIDE);
            }
        __syncthreads();                                 // the previous chunk's LDS reads are done
        for (int c = tid; c < nwin * 32; c += 256) {
            const int row = c >> 5, slot = c & 31;
            const long long src = ((long long)roi * S2 + wb + row) * C + slot * 8;
            const int dst = row * (C * 2) + ((slot ^ (row & 15)) << 4);
            *reinterpret_cast<cv_u32x4*>(&xs[0][dst]) = *reinterpret_cast<const cv_u32x4*>(feat_hi + src);
            if (X3) *reinterpret_cast<cv_u32x4*>(&xs[NIMG - 1][dst]) = *reinterpret_cast<const cv_u32x4*>(feat_lo + src);
        }
        if (tid < 32)
#pragma unroll
            for (int m = 0; m < NIMG; ++m) *reinterpret_cast<cv_u32x4*>(&xs[m][GW_ZERO * (C * 2) + (tid << 4)]) = cv_u32x4{0u, 0u, 0u, 0u};
        // cell coordinates of the chunk's 4 row tiles for this lane (cell = c0 + 16 i + fr)
        int cy[4], cx[4];
        bool cv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { const int cell = c0 + 16 * i + fr; cv[i] = cell < S2; cy[i] = cell / s; cx[i] = cell - cy[i] * s; }
        f32x4_t acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
            int src[4];
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int y = cy[it] + dy, x = cx[it] + dx;
                const bool ok = cv[it] && y >= 0 && y < s && x >= 0 && x < s;
                src[it] = ok ? y * s + x - wb : GW_ZERO;
            }
#pragma unroll
            for (int sk = 0; sk < 8; ++sk) {
                const int ks = tap * 8 + sk;
                if (ks + RING - 1 < 72) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        wqh[(sk + RING - 1) % RING][j].u = *reinterpret_cast<const uint4*>(Wh + w_off + (ks + RING - 1) * KS_STRIDE + j * JT_STRIDE);
                        if (X3) wql[(sk + RING - 1) % RING][j].u = *reinterpret_cast<const uint4*>(Wl + w_off + (ks + RING - 1) * KS_STRIDE + j * JT_STRIDE);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                Frag ah[4], al[4];
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int off = src[it] * (C * 2) + (((4 * sk + fg) ^ (src[it] & 15)) << 4);
                    ah[it].u = *reinterpret_cast<const uint4*>(&xs[0][off]);
                    if (X3) al[it].u = *reinterpret_cast<const uint4*>(&xs[NIMG - 1][off]);
                }
                if (X3) {
#pragma unroll
                    for (int it = 0; it < 4; ++it)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[it][j] = mfma_k16_16x16x32(al[it].u, wqh[sk % RING][j].u, acc[it][j]);
#pragma unroll
                    for (int it = 0; it < 4; ++it)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[it][j] = mfma_k16_16x16x32(ah[it].u, wql[sk % RING][j].u, acc[it][j]);
                }
#pragma unroll
                for (int it = 0; it < 4; ++it)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[it][j] = mfma_k16_16x16x32(ah[it].u, wqh[sk % RING][j].u, acc[it][j]);
            }
        }
        // bias + ReLU of the chunk's cells, each handed to the kernel: lane holds cells c0 + 16 i + 4 fg + r of column 64 wave + 16 j + fr
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = wave * 64 + 16 * j + fr;
            const float b = bs[n];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int cell = c0 + 16 * i + 4 * fg + r;
                    if (cell >= S2) continue;
                    ROI_CONV_WALK_CELL(relu_f(acc[i][j][r] + b), cell, n, j);
                }
        }
    }
