// Body of pe_x3_gate_kernel<MT> / pe_x3_gate_rows_kernel<MT> (pe_x3_gate.hip includes it once per kernel, so that the pe-only kernel keeps its
// instruction stream).  Reads: MT, the kernel parameter p; PX_GATE_ROWS: 1 = the key / value row outputs and the view filter r (PeGateRows).
    constexpr int KS1 = 6;                              // (names the steps of part 4 in the gated schedule; the gate itself has no depth)
    using S = Sched<KS1>;
    constexpr int T0 = S::first_of(4);
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM_G];
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
#if PX_GATE_ROWS
    const unsigned sel_mask = *r.sel.view_mask;         // a tile without a row of a cached view returns before the first barrier (block-uniform)
    if (!sel_tile_any(sel_mask, p.row_index, m0, M, lane, p.tab_period, r.sel)) return;
#endif
    // the feature rows of the tile (256 channels = 32 chunks per row, gathered through row_index): the block's first requests
    Stage<32, MT> fs;
    fs.load(p.Xmap, C, p.row_index, m0, M, tid);
    __builtin_amdgcn_sched_barrier(0);                 // (pe_x3_body.inc: without it hipcc sinks the row loads to fs.commit)
    const long long lo = (long long)lane * 8 + (long long)wave * CT * 512;
    const WBase w{{p.Wr_h + lo, p.Wr_l + lo}, {p.We_h + lo, p.We_l + lo}, {nullptr, nullptr}, {nullptr, nullptr}};
    XFrag wq[RING][CT], a[2][RT];
    ring_load<KS1, T0>(wq, w);
    ring_load<KS1, T0 + 1>(wq, w);
    if constexpr (RING > 3) ring_load<KS1, T0 + 2>(wq, w);
    if constexpr (RING > 4) ring_load<KS1, T0 + 3>(wq, w);
    if constexpr (RING > 5) ring_load<KS1, T0 + 4>(wq, w);
    if (tid < G_FLOATS / 4)                             // biases -> LDS: [br | be] as 128 float4
        *reinterpret_cast<float4*>(Bs + 4 * tid) = *reinterpret_cast<const float4*>(tid < 64 ? p.br + 4 * tid : p.be + 4 * (tid - 64));
    fs.commit(Ah, Al, tid);
    __syncthreads();
    const int n0 = wave * CT * 16 + 4 * fg;             // this lane's 4 output columns of column tile j start at n0 + 16 j
    f32x4_t acc[RT][CT];
    {
        // layer 1 of the gate
        f32x4_t acc1[RT][CT];
        zero_acc(acc1);
        steps<KS1, T0, 8>(acc1, wq, a, w, Ah, Al, fr, fg);
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            const int lcol = (wave * CT + j) * 16 + 4 * fg;
            const float4 bb = *reinterpret_cast<const float4*>(Bs + G_R + lcol);
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
    // read-back mapping of the output phase: lane -> (row r0 + 8 k, columns c4..c4+3 of 32); the row indices travel under layer 2
    constexpr int NK = BM / 8;
    const int c4 = (lane & 7) * 4, r0 = lane >> 3;
    int ri[NK], rq[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int m = min(m0 + 8 * k + r0, M - 1);
        ri[k] = p.row_index ? p.row_index[m] : m;
        rq[k] = ri[k] % p.tab_period;
    }
#if PX_GATE_ROWS
    const unsigned sel_taken = sel_rows(sel_mask, ri, p.tab_period, r.sel);
    typename MapElem<MT>::raw4 fvq[NK];                // the fp32 feature pieces: as loaded, widened where they are used
#endif
    // the table rows and the Q rows (row outputs: and the feature pieces) of the first 32 output columns are requested before the gate's second layer
    float4 tvq[NK], qvq[NK];
    auto request = [&](int jp) {
        const long long gcol = wave * CT * 16 + jp * 32 + c4;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            tvq[k] = *reinterpret_cast<const float4*>(p.sine_tab + (long long)rq[k] * C + gcol);
            qvq[k] = *reinterpret_cast<const float4*>(p.Q + (long long)rq[k] * C + gcol);
#if PX_GATE_ROWS
            fvq[k] = MapElem<MT>::ld4(p.Xmap + (long long)ri[k] * C + gcol);
#endif
        }
    };
    request(0);
    zero_acc(acc);
    steps<KS1, T0 + 8, 8>(acc, wq, a, w, Hh, Hl, fr, fg);
    // ---- pe = tab + Q * gate.  The sigmoid in place, then through a wave-private LDS tile [BM rows][32 columns] and out in whole 128-byte row pieces
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        const float4 eb = *reinterpret_cast<const float4*>(Bs + G_E + n0 + 16 * j);
#pragma unroll
        for (int i = 0; i < RT; ++i)
            // (accurate exp: this route is compared at fp32 rounding level)
            acc[i][j] = f32x4_t{1.f / (1.f + expf(-(acc[i][j][0] + eb.x))), 1.f / (1.f + expf(-(acc[i][j][1] + eb.y))),
                                1.f / (1.f + expf(-(acc[i][j][2] + eb.z))), 1.f / (1.f + expf(-(acc[i][j][3] + eb.w)))};
    }
    __syncthreads();                                   // all LDS images free: they become the waves' output tiles
    float* ot = reinterpret_cast<float*>(smem) + wave * (BM * OT_PITCH);
#pragma unroll
    for (int jp = 0; jp < CT / 2; ++jp) {               // 32 columns (two column tiles) at a time
        if (jp > 0) __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < RT; ++i)
                *reinterpret_cast<float4*>(ot + (16 * i + fr) * OT_PITCH + 16 * j + 4 * fg) =
                    make_float4(acc[i][2 * jp + j][0], acc[i][2 * jp + j][1], acc[i][2 * jp + j][2], acc[i][2 * jp + j][3]);
        __builtin_amdgcn_wave_barrier();               // the tile is read back by the same wave only
        const long long gcol = wave * CT * 16 + jp * 32 + c4;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int row = 8 * k + r0, m = m0 + row;
            const float4 g = *reinterpret_cast<const float4*>(ot + row * OT_PITCH + c4);
            const float4 v = gate_out(tvq[k], qvq[k], g);
#if !PX_GATE_ROWS
            if (m < M) *reinterpret_cast<float4*>(p.pe + (long long)(p.pe_at_index ? ri[k] : m) * C + gcol) = v;
#else
            if (m < M && ((sel_taken >> k) & 1u)) {
                // the output phase of pe_x3_body.inc on the same pe bits
                if (p.pe) *reinterpret_cast<float4*>(p.pe + (long long)(p.pe_at_index ? ri[k] : m) * C + gcol) = v;
                const float4 f = MapElem<MT>::widen(fvq[k]);
                uint2 h, l;
                split_k16x2(v.x + f.x, v.y + f.y, h.x, l.x);
                split_k16x2(v.z + f.z, v.w + f.w, h.y, l.y);
                *reinterpret_cast<uint2*>(r.Xk_hi + (long long)m * C + gcol) = h;
                if (r.lo8) *reinterpret_cast<unsigned int*>(reinterpret_cast<unsigned char*>(r.Xk_lo) + (long long)m * C + gcol) = lo8_pack4_flag(l.x, l.y, r.lo8_flag);
                else *reinterpret_cast<uint2*>(r.Xk_lo + (long long)m * C + gcol) = l;
                split_k16x2(f.x, f.y, h.x, l.x);
                split_k16x2(f.z, f.w, h.y, l.y);
                *reinterpret_cast<uint2*>(r.Xv_hi + (long long)m * C + gcol) = h;
                if (r.lo8) *reinterpret_cast<unsigned int*>(reinterpret_cast<unsigned char*>(r.Xv_lo) + (long long)m * C + gcol) = lo8_pack4_flag(l.x, l.y, r.lo8_flag);
                else *reinterpret_cast<uint2*>(r.Xv_lo + (long long)m * C + gcol) = l;
            }
#endif
        }
        if (jp + 1 < CT / 2) request(jp + 1);
    }
