// Body of pe_x3_kernel<MT> / pe_x3_depth_kernel<MT, KS1> (pe_x3_kernel.h includes it once per kernel, so that the 64-bin kernel keeps its name and its
// instruction stream).  Reads: MT, the constant KS1, S = Sched<KS1>, the kernel parameter p.
    constexpr int TOUCH_STEP = 128 / (int)sizeof(MT);   // elements per 128-byte cache line: the touch loads cover a row's lines
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];
    unsigned char* Ah = smem;
    unsigned char* Al = smem + IMG;
    unsigned char* Hh = smem + 2 * IMG;
    unsigned char* Hl = smem + 3 * IMG;
    float* Bs = reinterpret_cast<float*>(smem + 4 * IMG);
    int M = p.M;
    if (p.m_dev) { const int md = *p.m_dev; M = md < M ? md : M; }
    const int m0 = blockIdx.x * BM;
    if (m0 >= M) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
    PX_SEL_BLOCK();                                     // (pe_x3_sel.h: a tile without a taken row returns here; nothing in the unfiltered kernels)
    const long long lo = (long long)lane * 8 + (long long)wave * CT * 512;
    const WBase w{{p.Wr_h + lo, p.Wr_l + lo}, {p.We_h + lo, p.We_l + lo}, {p.W1a_h + lo, p.W1a_l + lo}, {p.W1b_h + lo, p.W1b_l + lo}};
    XFrag wq[RING][CT], a[2][RT];
    float touch0 = 0.f, touch1 = 0.f;
    PX_STAMP(0);
    ring_load<KS1, 0>(wq, w);
    ring_load<KS1, 1>(wq, w);
    if constexpr (RING > 3) ring_load<KS1, 2>(wq, w);
    if constexpr (RING > 4) ring_load<KS1, 3>(wq, w);
    if constexpr (RING > 5) ring_load<KS1, 4>(wq, w);
    {
        // biases -> LDS: [br | be | b1a | b1b] as 448 float4
        constexpr int NB = (B_FLOATS / 4 + NTHR - 1) / NTHR;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int t = tid + NTHR * i;
            if (t < B_FLOATS / 4) {
                const float* src = t < 64 ? p.br + 4 * t : t < 128 ? p.be + 4 * (t - 64) : t < 384 ? p.b1a + 4 * (t - 128) : p.b1b + 4 * (t - 384);
                *reinterpret_cast<float4*>(Bs + 4 * t) = *reinterpret_cast<const float4*>(src);
            }
        }
        // the frustum rows of the tile (32 KS1 channels = 4 KS1 chunks per row; 192 = 24 chunks at 64 bins), fp32 -> hi / lo images
        Stage<4 * KS1> st;
        st.load(p.A1, 32 * KS1, nullptr, m0, M, tid);
        st.commit(Ah, Al, tid);
    }
#if MV2D_PX_TOUCH == 1
    PX_TOUCH_ISSUE();
#endif
    __syncthreads();
    PX_STAMP(1);
    const int n0 = wave * CT * 16 + 4 * fg;             // this lane's 4 output columns of column tile j start at n0 + 16 j
    f32x4_t accf[RT][CT];                               // P1 = position_encoder(A1), bias added at the end

    // ---- 1. P1 in four parts of 256 hidden columns
    zero_acc(accf);
    layer1<KS1, 0>(wq, a, w, Ah, Al, Hh, Hl, Bs + B_1A, wave, fr, fg);
    PX_STAMP(2);
    steps<KS1, S::first_of(0) + KS1, 8>(accf, wq, a, w, Hh, Hl, fr, fg);
    PX_STAMP(3);
    layer1<KS1, 1>(wq, a, w, Ah, Al, Hh, Hl, Bs + B_1A + 256, wave, fr, fg);
    PX_STAMP(4);
    steps<KS1, S::first_of(1) + KS1, 8>(accf, wq, a, w, Hh, Hl, fr, fg);
    PX_STAMP(5);
#if MV2D_PX_TOUCH == 2
    PX_TOUCH_ISSUE();
#endif
    layer1<KS1, 2>(wq, a, w, Ah, Al, Hh, Hl, Bs + B_1A + 512, wave, fr, fg);
    PX_STAMP(6);
    steps<KS1, S::first_of(2) + KS1, 8>(accf, wq, a, w, Hh, Hl, fr, fg);
    PX_STAMP(7);
    // the feature rows of the tile (256 channels = 32 chunks per row, gathered through row_index) are requested a whole part ahead: they travel
    // under the MFMAs of layer 1 (stamps of the first version: 22 k of a block's 145 k cycles waited for them right here)
    Stage<32, MT> fs;
    fs.load(p.Xmap, C, p.row_index, m0, M, tid);
#ifndef MV2D_PX_ROUND5_STAGE
    __builtin_amdgcn_sched_barrier(0);                 // (without it hipcc sinks the 16 row loads to fs.commit below: 16 dependent round trips per block, tools/isa_waits.sh)
#endif
#if MV2D_PX_TOUCH
    asm volatile("" ::"v"(touch0), "v"(touch1));      // the touch loads are complete at the latest here (their lines sit in L2 for the loads above)
#endif
    layer1<KS1, 3>(wq, a, w, Ah, Al, Hh, Hl, Bs + B_1A + 768, wave, fr, fg);        // after its barrier nobody reads the frustum images any more
    PX_STAMP(8);
    fs.commit(Ah, Al, tid);                            // other waves may still run the last layer 2 (hidden images only)
    PX_STAMP(9);
    steps<KS1, S::first_of(3) + KS1, 8>(accf, wq, a, w, Hh, Hl, fr, fg);
    PX_STAMP(10);
    __syncthreads();                                   // the feature tile is in the A images (and the last layer 2 is done with the hidden tile)
    PX_STAMP(11);
    // ---- 2. the gate
    f32x4_t acc[RT][CT];
    {
        // layer 1 of the gate: no barrier needed in front of its stores (the barrier above), P = 4
        f32x4_t acc1[RT][CT];
        zero_acc(acc1);
        steps<KS1, S::first_of(4), 8>(acc1, wq, a, w, Ah, Al, fr, fg);
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            const int lcol = (wave * CT + j) * 16 + 4 * fg;
            const float4 bb = *reinterpret_cast<const float4*>(Bs + B_R + lcol);
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                uint2 hv, lv;
                split4(relu_f(acc1[i][j][0] + bb.x), relu_f(acc1[i][j][1] + bb.y), relu_f(acc1[i][j][2] + bb.z), relu_f(acc1[i][j][3] + bb.w), hv, lv);
                const int off = (16 * i + fr) * PITCH + (((lcol >> 3) ^ fr) << 4) + (lcol & 4) * 2;
                *reinterpret_cast<uint2*>(Hh + off) = hv;
                *reinterpret_cast<uint2*>(Hl + off) = lv;
            }
        }
        __syncthreads();
    }
    PX_STAMP(12);
    // read-back mapping of the output phase: lane -> (row r0 + 8 k, columns c4..c4+3 of 32); the row indices travel under layer 2
    constexpr int NK = BM / 8;
    const int c4 = (lane & 7) * 4, r0 = lane >> 3;
    int ri[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int m = min(m0 + 8 * k + r0, M - 1);
        ri[k] = p.row_index ? p.row_index[m] : m;
    }
    PX_SEL_ROWS();
    // the table rows (and, T path, the fp32 feature rows) of the first 32 output columns are requested before the gate's second layer
    const bool rows16 = p.Xk_hi != nullptr;
    float4 tvq[NK];
    typename MapElem<MT>::raw4 fvq[NK];                // as loaded, widened where it is used
    auto request = [&](int jp) {
        const long long gcol = wave * CT * 16 + jp * 32 + c4;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            tvq[k] = *reinterpret_cast<const float4*>(p.sine_tab + (long long)(ri[k] % p.tab_period) * C + gcol);
            if (rows16) fvq[k] = MapElem<MT>::ld4(p.Xmap + (long long)ri[k] * C + gcol);
        }
    };
    request(0);
    zero_acc(acc);
    steps<KS1, S::first_of(4) + 8, 8>(acc, wq, a, w, Hh, Hl, fr, fg);
    PX_STAMP(13);
    // ---- 3. pe = tab + (P1 + b) * gate; T path: Xk = pe + feat, Xv = feat as key16 hi + lo pairs.  Through a wave-private LDS tile
    // [BM rows][32 columns], then whole 128-byte row pieces.  The sigmoid in place, the bias of P1:
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        const float4 eb = *reinterpret_cast<const float4*>(Bs + B_E + n0 + 16 * j);
        const float4 fb = *reinterpret_cast<const float4*>(Bs + B_1B + n0 + 16 * j);
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            // (accurate exp: this route is compared at fp32 rounding level)
            const f32x4_t g{1.f / (1.f + expf(-(acc[i][j][0] + eb.x))), 1.f / (1.f + expf(-(acc[i][j][1] + eb.y))),
                            1.f / (1.f + expf(-(acc[i][j][2] + eb.z))), 1.f / (1.f + expf(-(acc[i][j][3] + eb.w)))};
            accf[i][j] = f32x4_t{(accf[i][j][0] + fb.x) * g[0], (accf[i][j][1] + fb.y) * g[1], (accf[i][j][2] + fb.z) * g[2], (accf[i][j][3] + fb.w) * g[3]};
        }
    }
    __syncthreads();                                   // all LDS images free: they become the waves' output tiles
    PX_STAMP(14);
    float* ot = reinterpret_cast<float*>(smem) + wave * (BM * OT_PITCH);
#pragma unroll
    for (int jp = 0; jp < CT / 2; ++jp) {               // 32 columns (two column tiles) at a time
        if (jp > 0) __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < RT; ++i)
                *reinterpret_cast<float4*>(ot + (16 * i + fr) * OT_PITCH + 16 * j + 4 * fg) =
                    make_float4(accf[i][2 * jp + j][0], accf[i][2 * jp + j][1], accf[i][2 * jp + j][2], accf[i][2 * jp + j][3]);
        __builtin_amdgcn_wave_barrier();               // the tile is read back by the same wave only
        const long long gcol = wave * CT * 16 + jp * 32 + c4;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int row = 8 * k + r0, m = m0 + row;
            float4 v = *reinterpret_cast<const float4*>(ot + row * OT_PITCH + c4);
            const float4 tv = tvq[k];
            v = make_float4(v.x + tv.x, v.y + tv.y, v.z + tv.z, v.w + tv.w);
            if (m < M && PX_SEL_TAKEN(k)) {
                if (p.pe) *reinterpret_cast<float4*>(p.pe + (long long)(p.pe_at_index ? ri[k] : m) * C + gcol) = v;
                if (rows16) {
                    const float4 f = MapElem<MT>::widen(fvq[k]);
                    uint2 h, l;
                    split_k16x2(v.x + f.x, v.y + f.y, h.x, l.x);
                    split_k16x2(v.z + f.z, v.w + f.w, h.y, l.y);
                    *reinterpret_cast<uint2*>(p.Xk_hi + (long long)m * C + gcol) = h;
                    if (p.lo8) *reinterpret_cast<unsigned int*>(reinterpret_cast<unsigned char*>(p.Xk_lo) + (long long)m * C + gcol) = lo8_pack4_flag(l.x, l.y, p.lo8_flag);
                    else *reinterpret_cast<uint2*>(p.Xk_lo + (long long)m * C + gcol) = l;
                    split_k16x2(f.x, f.y, h.x, l.x);
                    split_k16x2(f.z, f.w, h.y, l.y);
                    *reinterpret_cast<uint2*>(p.Xv_hi + (long long)m * C + gcol) = h;
                    if (p.lo8) *reinterpret_cast<unsigned int*>(reinterpret_cast<unsigned char*>(p.Xv_lo) + (long long)m * C + gcol) = lo8_pack4_flag(l.x, l.y, p.lo8_flag);
                    else *reinterpret_cast<uint2*>(p.Xv_lo + (long long)m * C + gcol) = l;
                }
            }
        }
        if (jp + 1 < CT / 2) request(jp + 1);
        PX_STAMP(15 + jp);
    }
