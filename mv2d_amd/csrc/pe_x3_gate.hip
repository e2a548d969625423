// The GATE of the split-precision PE block alone (pe_x3_kernel.h, from "---- 2. the gate" onward) on a cached frustum MLP:
//   G  = sigmoid(conv_expand(relu(conv_reduce(feat))))          256 -> 256 -> 256      (MU/pe.py:36-48, 162-166)
//   pe = tab[position] + Q[position] * G                         Q = position_encoder(A1) + b1b, constant per (weights, padding geometry, camera matrices)
// Q is what the gate-less kernel (pe_x3_nogate_kernel on a zero table) writes for all positions of one sample: the rounded P1 + b1b of the gated
// kernel bit for bit, so pe is bit for bit the gated kernel's (the product and the table sum stay two roundings: gate_out below).  The 16 k-steps
// of part 4 of the gated schedule run on the same ring, the same LDS images and in the same MFMA order; parts 0..3 (56 of 72 k-steps at 64 bins), the
// frustum rows and the W1a / W1b streams are gone.  The feature tile is requested first thing in the block (nothing to hide it under any more), the Q and
// table rows of an output half where the gated kernel requests its table rows.  One instance per map format; no depth instances (the depth only
// shapes Q); pe output only (the S path reads nothing else).
#include "pe_x3_kernel.h"

template <class MT>
struct PeGateParamsT {
    const float* Q; const MT* Xmap; const int* row_index; const int* m_dev; int M;
    const unsigned short* Wr_h; const unsigned short* Wr_l; const float* br; const unsigned short* We_h; const unsigned short* We_l; const float* be;
    const float* sine_tab; int tab_period;
    float* pe; int pe_at_index;
};

namespace {

enum { G_R = 0, G_E = 256, G_FLOATS = 512 };
constexpr int SMEM_G = 4 * IMG + G_FLOATS * 4;

// tab + q * g in TWO roundings (the gated kernel rounds (P1 + b) * g on its way through LDS, then adds the table row): no contraction to an FMA
__device__ __forceinline__ float4 gate_out(const float4& tv, const float4& q, const float4& g) {
#pragma clang fp contract(off)
    const float4 pr = make_float4(q.x * g.x, q.y * g.y, q.z * g.z, q.w * g.w);
    return make_float4(pr.x + tv.x, pr.y + tv.y, pr.z + tv.z, pr.w + tv.w);
}

}  // namespace

template <class MT>
__global__ __launch_bounds__(NTHR, 1) void pe_x3_gate_kernel(PeGateParamsT<MT> p) {
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
    // the table rows and the Q rows of the first 32 output columns are requested before the gate's second layer
    float4 tvq[NK], qvq[NK];
    auto request = [&](int jp) {
        const long long gcol = wave * CT * 16 + jp * 32 + c4;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            tvq[k] = *reinterpret_cast<const float4*>(p.sine_tab + (long long)rq[k] * C + gcol);
            qvq[k] = *reinterpret_cast<const float4*>(p.Q + (long long)rq[k] * C + gcol);
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
            if (m < M) *reinterpret_cast<float4*>(p.pe + (long long)(p.pe_at_index ? ri[k] : m) * C + gcol) = v;
        }
        if (jp + 1 < CT / 2) request(jp + 1);
    }
}

// C-ABI: include/mv2d_hip.h
template <class MT>
static void pe_gate_launch(const float* Q, const void* Xmap, const int* row_index, const int* m_dev, int M, const void* Wr_hi, const void* Wr_lo, const float* br,
                           const void* We_hi, const void* We_lo, const float* be, const float* sine_tab, int tab_period, float* pe, int pe_at_index, void* stream) {
    PeGateParamsT<MT> p{Q, (const MT*)Xmap, row_index, m_dev, M, (const unsigned short*)Wr_hi, (const unsigned short*)Wr_lo, br, (const unsigned short*)We_hi,
                        (const unsigned short*)We_lo, be, sine_tab, tab_period, pe, pe_at_index};
    hipLaunchKernelGGL(pe_x3_gate_kernel<MT>, dim3(cdiv(M, BM)), dim3(NTHR), 0, (hipStream_t)stream, p);
}

extern "C" int mv2d_pe_gate_x3(const float* Q, const void* Xmap, const int* row_index, const int* m_dev, int M,
                               const void* Wr_hi, const void* Wr_lo, const float* br, const void* We_hi, const void* We_lo, const float* be,
                               const float* sine_tab, int tab_period, float* pe, void* Xk_hi, void* Xk_lo, void* Xv_hi, void* Xv_lo, int pe_at_index,
                               int map_fmt, void* stream) {
    MV2D_CHECK_ARG(!Xk_hi && !Xk_lo && !Xv_hi && !Xv_lo, "mv2d_pe_gate_x3: no key / value row outputs (pe only: run mv2d_pe_fused_x3_k for the rows)");
    MV2D_CHECK_ARG(Q && Xmap && Wr_hi && Wr_lo && br && We_hi && We_lo && be && sine_tab && pe, "mv2d_pe_gate_x3: null pointer");
    MV2D_CHECK_ARG(!pe_at_index || row_index, "mv2d_pe_gate_x3: pe_at_index needs row_index");
    MV2D_CHECK_ARG(M >= 0 && tab_period > 0, "mv2d_pe_gate_x3: M must be >= 0 and tab_period > 0");
    MV2D_CHECK_ARG(map_fmt >= 0 && map_fmt <= 2, "mv2d_pe_gate_x3: map_fmt is 0 (fp32), 1 (fp16) or 2 (bf16)");
    MV2D_CHECK_ARG(((uintptr_t)Q & 15) == 0 && ((uintptr_t)Xmap & (map_fmt ? 7 : 15)) == 0 && ((uintptr_t)sine_tab & 15) == 0 && ((uintptr_t)pe & 15) == 0,
                   "mv2d_pe_gate_x3: rows must be 16-byte aligned (a 16-bit map: 8-byte)");
    if (M == 0) return MV2D_OK;
    MV2D_MAP_DISPATCH(map_fmt, pe_gate_launch<MT>(Q, Xmap, row_index, m_dev, M, Wr_hi, Wr_lo, br, We_hi, We_lo, be, sine_tab, tab_period, pe, pe_at_index, stream));
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}
