// The PE block of the key side in SPLIT PRECISION (index-exact route; gfx950 / CDNA4, wave64), one launch:
//   P1 = position_encoder(A1)                                   192 -> 1024 -> 256     (MU/pe.py:64-77, 158-160)
//   G  = sigmoid(conv_expand(relu(conv_reduce(feat))))          256 -> 256 -> 256      (MU/pe.py:36-48, 162-166)
//   pe = tab[position] + P1 * G                                  tab = adapt_pos3d(sine) + bias, constant per (weights, padding geometry)
//   T path: key rows Xk = pe + feat and value rows Xv = feat, each as a key16 hi + lo pair (what xattn_tile_kernel<.., XLO> gathers)
// on UNROUNDED fp32 inputs (frustum rows from pe_inputs_kernel<true>, feature rows read from the map): every product is
// a_hi w_hi + a_lo w_hi + a_hi w_lo on v_mfma_f32_16x16x32_bf16 with fp32 accumulation (operands split into bf16 hi / lo, 2^-17 per operand,
// the hidden layer split when it is written to LDS) -- the arithmetic of the K-concatenated GEMM chain it replaces
// ([a_hi | a_lo | a_hi] . [w_hi | w_hi | w_lo]^T on the plain tile GEMM, round 3), which moved the 1024-wide hidden layer through HBM as
// [hi | lo | hi] (860 MB out + 860 MB back per 16-sample launch) in four launches + two operand-split passes + two row-split passes:
// 977 + 116 us (S path) / 1733 + 202 + 237 us (T path) per 16-sample launch.
//
// Structure = pe_tab_kernel's (pe_tab96.hip) 64-row shape: 4 waves, wave w owns column tiles 4w..4w+3 of every 256-column part for all 4 row
// tiles, fragment-major weights streamed straight from L2 through a register ring (hi and lo streams), the hidden layer in parts of 256
// columns through LDS, the gate LAST.  hi and lo images of the input tile and of the hidden tile live side by side in LDS (128 KB): one
// block per CU, one wave per SIMD (<= 512 registers), 48 MFMAs per k-step per wave -- the kernel is matrix-pipe bound by construction
// (3 x the MFMAs of the default kernel on the same loads).
// (this header: the kernel; pe_x3.hip: the 64-bin instance and the C entries; pe_x3_d1.hip / pe_x3_d2.hip: the instances of the other depths;
// pe_x3_ng1.hip / pe_x3_ng2.hip: the instances of the gate-less kernel pe_x3_nogate_kernel<MT, KS1>, the PE built with with_fpe=False)
#pragma once
#include "common.h"

#ifdef MV2D_PX_TRACE
static __device__ long long g_px_trace[32];
#define PX_STAMP(i) do { if (blockIdx.x == MV2D_PX_TRACE && threadIdx.x == 0) g_px_trace[i] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#else
#define PX_STAMP(i) do {} while (0)
#endif

template <class MT>         // MT: element type of the feature map Xmap (common.h MapElem)
struct PeX3ParamsT {
    const float* A1; const MT* Xmap; const int* row_index; const int* m_dev; int M;
    const unsigned short* W1a_h; const unsigned short* W1a_l; const float* b1a; const unsigned short* W1b_h; const unsigned short* W1b_l; const float* b1b;
    const unsigned short* Wr_h; const unsigned short* Wr_l; const float* br; const unsigned short* We_h; const unsigned short* We_l; const float* be;
    const float* sine_tab; int tab_period;
    float* pe; unsigned short* Xk_hi; unsigned short* Xk_lo; unsigned short* Xv_hi; unsigned short* Xv_lo;
    int lo8;                                                 // the lo row outputs are 256-byte e4m3 rows (common.h "lo8")
    int* lo8_flag;                                           // |= 1 when a lo remainder leaves the e4m3 range (may be NULL)
    int pe_at_index;                                         // pe row m is written at row row_index[m] (a position-indexed map) instead of row m
};

// The instances for the other depths are compiled in translation units of their own (pe_x3_d1.hip: KS1 = 1 .. 4, pe_x3_d2.hip: KS1 = 5, 7, 8; a build
// compiles the three files side by side): each launches pe_x3_depth_kernel<MT, ks1> on `blocks` blocks, or returns false for a ks1 it does not hold.
template <class MT> bool mv2d_px_launch_d1(const PeX3ParamsT<MT>& p, int ks1, int blocks, hipStream_t stream);
template <class MT> bool mv2d_px_launch_d2(const PeX3ParamsT<MT>& p, int ks1, int blocks, hipStream_t stream);
// The same for the gate-less kernel pe_x3_nogate_kernel<MT, ks1> (pe_x3_ng1.hip: KS1 = 1 .. 4, pe_x3_ng2.hip: KS1 = 5 .. 8); p's Wr / We / br / be are not read.
template <class MT> bool mv2d_px_launch_ng1(const PeX3ParamsT<MT>& p, int ks1, int blocks, hipStream_t stream);
template <class MT> bool mv2d_px_launch_ng2(const PeX3ParamsT<MT>& p, int ks1, int blocks, hipStream_t stream);

namespace {

constexpr int C = 256;
constexpr int PITCH = 512;                                  // bytes per row of an LDS image (256 bf16), 16-byte chunk c of row r at c ^ (r & 15)
#ifndef MV2D_PX_RING
#define MV2D_PX_RING 3
#endif
constexpr int RT = 4, NW = 4, CT = 4, BM = 16 * RT, NTHR = 64 * NW, RING = MV2D_PX_RING;
constexpr int IMG = BM * PITCH;                             // one 64-row image: 32 KB
enum { B_R = 0, B_E = 256, B_1A = 512, B_1B = 1536, B_FLOATS = 1792 };
constexpr int OT_PITCH = 36;                                // floats per row of a wave's output tile [BM][32 columns]
constexpr int SMEM = 4 * IMG + B_FLOATS * 4;                // A hi | A lo | H hi | H lo | biases = 135 KB
static_assert(NW * BM * OT_PITCH * 4 <= 4 * IMG, "the waves' output tiles fit into the LDS images they replace");

typedef q16x8_t px_bf16x8;      // common.h "q16": fp16 pairs since round 5
struct XFrag { uint4 h, l; };

// ---- the k-steps of a block as one compile-time schedule (pe_tab96.hip): parts 0..3 = hidden columns 256 p .. of the frustum MLP
// (KS1 + 8 steps each), part 4 = the gate (8 + 8 steps).  Step T consumes CT weight fragments of the hi and of the lo stream.
// KS1 = Kp / 32 = first-layer k-steps of the frustum MLP: its rows are 3 * depth_num columns zero-padded to Kp = 32 * ceil(3 * depth_num / 32)
// (1 .. 8 for depth_num 8 .. 80; 6 = the 64 bins of the shipped configs: 72 steps).  The ring runs RING - 1 steps ahead of the MFMAs whatever
// layer those steps belong to (at KS1 = 1 the prologue's second load is already a W1b fragment); the hidden-image barriers of layer1 order LDS
// accesses only, so they hold for every KS1.
// GATE = false (pe_x3_nogate_kernel): the schedule ends after part 3 -- NSTEP = 4 PER, no step belongs to a part 4, the ring stops at the end of W1b.
template <int KS1, bool GATE = true> struct Sched {
    static_assert(KS1 >= 1 && KS1 <= 8, "the frustum image is at most the 256 columns of an LDS image");
    static constexpr int PER = KS1 + 8, NSTEP = 4 * PER + (GATE ? 16 : 0);
    static constexpr int part_of(int T) { return T < 4 * PER ? T / PER : 4; }          // (4 only for T >= 4 PER: never below NSTEP without the gate)
    static constexpr int first_of(int p) { return p * PER; }
    static constexpr int ks1_of(int p) { return p == 4 ? 8 : KS1; }
};

struct WBase { const unsigned short* wr[2]; const unsigned short* we[2]; const unsigned short* w1a[2]; const unsigned short* w1b[2]; };   // [hi, lo], + lane * 8 + wave * CT tiles

template <int KS1, int T, bool GATE = true>
__device__ __forceinline__ long long step_off() {
    using S = Sched<KS1, GATE>;
    constexpr int p = S::part_of(T), t = T - S::first_of(p), ks1 = S::ks1_of(p);
    static_assert(GATE || p < 4, "the gate-less schedule has no part 4");
    if constexpr (p == 4) {
        if constexpr (t < ks1) return (long long)(t * 16) * 512;                               // Wr  [ks][16 tiles]
        else return (long long)((t - ks1) * 16) * 512;                                         // We  [ks][16 tiles]
    } else {
        if constexpr (t < ks1) return (long long)(t * 64 + p * 16) * 512;                      // W1a [ks][64 tiles], this part's 16 tiles
        else return (long long)((p * 8 + (t - ks1)) * 16) * 512;                               // W1b [32 k-steps][16 tiles]
    }
}
template <int KS1, int T, bool GATE = true>
__device__ __forceinline__ const unsigned short* step_base(const WBase& w, int part) {
    using S = Sched<KS1, GATE>;
    constexpr int p = S::part_of(T), t = T - S::first_of(p), ks1 = S::ks1_of(p);
    if constexpr (p == 4) return t < ks1 ? w.wr[part] : w.we[part];
    else return t < ks1 ? w.w1a[part] : w.w1b[part];
}

template <int KS1, int T, bool GATE = true>
__device__ __forceinline__ void ring_load(XFrag (&wq)[RING][CT], const WBase& w) {
    if constexpr (T < Sched<KS1, GATE>::NSTEP) {
        const unsigned short* ph = step_base<KS1, T, GATE>(w, 0) + step_off<KS1, T, GATE>();
        const unsigned short* pl = step_base<KS1, T, GATE>(w, 1) + step_off<KS1, T, GATE>();
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            wq[T % RING][j].h = *reinterpret_cast<const uint4*>(ph + 512 * j);
            wq[T % RING][j].l = *reinterpret_cast<const uint4*>(pl + 512 * j);
        }
    }
}

__device__ __forceinline__ void load_a(XFrag (&a)[RT], const unsigned char* Lh, const unsigned char* Ll, int kstep, int fr, int fg) {
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const int off = (16 * i + fr) * PITCH + (((4 * kstep + fg) ^ fr) << 4);
        a[i].h = *reinterpret_cast<const uint4*>(Lh + off);
        a[i].l = *reinterpret_cast<const uint4*>(Ll + off);
    }
}

// N k-steps of one layer.  The activation fragments of step K + 1 are read from LDS before the MFMAs of step K issue.
template <int KS1, int T0, int N, int K = 0, bool GATE = true>
__device__ __forceinline__ void steps(f32x4_t (&acc)[RT][CT], XFrag (&wq)[RING][CT], XFrag (&a)[2][RT], const WBase& w, const unsigned char* Lh,
                                      const unsigned char* Ll, int fr, int fg) {
    if constexpr (K < N) {
        if constexpr (K == 0) load_a(a[0], Lh, Ll, 0, fr, fg);
        ring_load<KS1, T0 + K + RING - 1, GATE>(wq, w);
        if constexpr (K + 1 < N) load_a(a[(K + 1) & 1], Lh, Ll, K + 1, fr, fg);
        __builtin_amdgcn_sched_barrier(0);             // the loads stay ahead of the MFMAs
        // product-major: 16 independent MFMAs between two that accumulate into the same tile (a dependent MFMA waits ~8 passes for its input)
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int j = 0; j < CT; ++j) {
                    const XFrag& wf = wq[(T0 + K) % RING][j];
                    const XFrag& af = a[K & 1][i];
                    acc[i][j] = mfma_q16_16x16x32(t == 0 ? wf.l : wf.h, t == 1 ? af.l : af.h, acc[i][j]);
                }
        __builtin_amdgcn_sched_barrier(0);
        steps<KS1, T0, N, K + 1, GATE>(acc, wq, a, w, Lh, Ll, fr, fg);
    }
}

__device__ __forceinline__ void zero_acc(f32x4_t (&acc)[RT][CT]) {
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ void split4(float a, float b, float c, float d, uint2& hi, uint2& lo) {
    split_q16x2(a, b, hi.x, lo.x);
    split_q16x2(c, d, hi.y, lo.y);
}

// layer 1 of part P into the hidden images: lane (fr, fg) holds hidden columns lcol..lcol+3 of row 16 i + fr -> bias, ReLU, hi / lo split,
// two 8-byte writes.  A barrier before the stores waits for the previous part's layer 2 (one hidden buffer), one after completes the tile.
template <int KS1, int P, bool GATE = true>
__device__ __forceinline__ void layer1(XFrag (&wq)[RING][CT], XFrag (&a)[2][RT], const WBase& w, const unsigned char* Ah, const unsigned char* Al,
                                       unsigned char* Hh, unsigned char* Hl, const float* bias /* LDS, this part's 256 */, int wave, int fr, int fg) {
    f32x4_t acc1[RT][CT];
    zero_acc(acc1);
    steps<KS1, Sched<KS1, GATE>::first_of(P), KS1, 0, GATE>(acc1, wq, a, w, Ah, Al, fr, fg);
    if constexpr (P > 0 && P < 4) __syncthreads();   // (the gate's layer 1 follows a block barrier anyway)
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        const int lcol = (wave * CT + j) * 16 + 4 * fg;
        const float4 bb = *reinterpret_cast<const float4*>(bias + lcol);
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

// fp32 rows -> hi / lo LDS images: NCH 16-byte chunks (8 columns) per row, thread t moves float4 pieces (half a chunk each).  Two phases, so
// that the loads can be in flight under MFMA work: stage_load issues them, stage_commit splits and writes the images.
// ET: element type of the rows (float, or a 16-bit feature map: the pieces stay in their 8-byte form until commit widens and splits them)
template <int NCH, class ET = float>
struct Stage {
    static constexpr int PIECES = BM * NCH * 2, PER = PIECES / NTHR;
    static_assert(PIECES % NTHR == 0, "");
    typename MapElem<ET>::raw4 v[PER];
    __device__ __forceinline__ void load(const ET* __restrict__ src, long long ld, const int* __restrict__ ridx, int m0, int M, int tid) {
        // all row indices first, then all rows: written as one loop, the compiler waited for index i AND row i - 1 (vmcnt(0)) in front of every row -- PER
        // dependent round trips per block instead of two (round 6, tools/isa_waits.sh)
#ifdef MV2D_PX_ROUND5_STAGE      // (timing A/B: the round-5 form)
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = tid + NTHR * i, row = c / (2 * NCH), piece = c - row * (2 * NCH);
            const int m = min(m0 + row, M - 1);
            const long long r = ridx ? ridx[m] : m;
            v[i] = MapElem<ET>::ld4(src + r * ld + piece * 4);
        }
#else
        int r[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = tid + NTHR * i, row = c / (2 * NCH);
            const int m = min(m0 + row, M - 1);
            r[i] = ridx ? ridx[m] : m;
        }
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = tid + NTHR * i, row = c / (2 * NCH), piece = c - row * (2 * NCH);
            v[i] = MapElem<ET>::ld4(src + (long long)r[i] * ld + piece * 4);
        }
#endif
    }
    __device__ __forceinline__ void commit(unsigned char* Lh, unsigned char* Ll, int tid) const {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = tid + NTHR * i, row = c / (2 * NCH), piece = c - row * (2 * NCH), chunk = piece >> 1;
            uint2 hv, lv;
            const float4 f = MapElem<ET>::widen(v[i]);
            split4(f.x, f.y, f.z, f.w, hv, lv);
            const int off = row * PITCH + ((chunk ^ (row & 15)) << 4) + (piece & 1) * 8;
            *reinterpret_cast<uint2*>(Lh + off) = hv;
            *reinterpret_cast<uint2*>(Ll + off) = lv;
        }
    }
};

// The feature rows of a tile are a GATHER (64 rows x 1 KB through row_index) that all blocks of a round request at the same moment; loads return in
// order, so the weight-ring wait behind them stalls for the whole gather (round-5 stamps: 18 k of a block's 141 k cycles in front of layer 1 of
// part 3).  MV2D_PX_TOUCH: every thread reads ONE word of two of the tile's 512 cache lines early -- 1 = in the prologue (the frustum rows are waited
// for there anyway), 2 = in front of part 2 -- so that the real loads find their lines in L2.
#ifndef MV2D_PX_TOUCH
#define MV2D_PX_TOUCH 2
#endif
#define PX_TOUCH_ISSUE()                                                                                   \
    do {                                                                                                   \
        const int c0_ = tid, c1_ = tid + NTHR;                                                             \
        const int ma_ = min(m0 + (c0_ >> 3), M - 1), mb_ = min(m0 + (c1_ >> 3), M - 1);                    \
        const long long ra_ = p.row_index ? p.row_index[ma_] : ma_, rb_ = p.row_index ? p.row_index[mb_] : mb_; \
        touch0 = MapElem<MT>::ld1(p.Xmap + ra_ * C + (c0_ & (C / TOUCH_STEP - 1)) * TOUCH_STEP);                              \
        touch1 = MapElem<MT>::ld1(p.Xmap + rb_ * C + (c1_ & (C / TOUCH_STEP - 1)) * TOUCH_STEP);                              \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
    } while (0)

// The hooks of the view filter in pe_x3_body.inc (pe_x3_sel.h fills them in for pe_x3_sel_kernel): nothing in the kernels of this header
#define PX_SEL_BLOCK() do {} while (0)
#define PX_SEL_ROWS() do {} while (0)
#define PX_SEL_TAKEN(k) true

// KS1 = 6 (the shipped 64 bins, A1 rows of 192 columns) keeps the kernel's name; the other depths are pe_x3_depth_kernel<MT, KS1> (A1 rows of pitch 32 KS1)
template <class MT>
__global__ __launch_bounds__(NTHR, 1) void pe_x3_kernel(PeX3ParamsT<MT> p) {
    constexpr int KS1 = 6;
    using S = Sched<KS1>;
#include "pe_x3_body.inc"
}

template <class MT, int KS1>
__global__ __launch_bounds__(NTHR, 1) void pe_x3_depth_kernel(PeX3ParamsT<MT> p) {
    using S = Sched<KS1>;
#include "pe_x3_body.inc"
}

// The PE built with with_fpe=False (MU/pe.py:81-82, 158-159: no fpe submodule): pe = tab[position] + position_encoder(A1), no gate.  Parts 0..3 are the
// calls of the body above in the same order on the same accumulator (P1 is bit for bit the gated kernel's), the schedule ends there (Sched<KS1, false>:
// 4 (KS1 + 8) k-steps, 56 instead of 72 at 64 bins; the ring stops after the last W1b fragment), the feature tile is never staged into the A images, Wr / We
// / br / be are never read, the bias block in LDS is [b1a | b1b].  The feature rows are read in the output phase only, and only for the key / value row
// outputs: without them (S path) Xmap may be NULL.  No early touch of the tile's feature lines (MV2D_PX_TOUCH above): measured with and without on the
// rows of a 16-sample cfg3_t launch it moves the launch by -1.0 % .. +0.6 %, inside the spread of repeats (profiles/pe_options_kernel_stats.txt).
enum { NG_1A = 0, NG_1B = 1024, NG_FLOATS = 1280 };
constexpr int SMEM_NG = 4 * IMG + NG_FLOATS * 4;

template <class MT, int KS1>
__global__ __launch_bounds__(NTHR, 1) void pe_x3_nogate_kernel(PeX3ParamsT<MT> p) {
    using S = Sched<KS1, false>;
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM_NG];
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
    const long long lo = (long long)lane * 8 + (long long)wave * CT * 512;
    const WBase w{{nullptr, nullptr}, {nullptr, nullptr}, {p.W1a_h + lo, p.W1a_l + lo}, {p.W1b_h + lo, p.W1b_l + lo}};
    XFrag wq[RING][CT], a[2][RT];
    const bool rows16 = p.Xk_hi != nullptr;
    ring_load<KS1, 0, false>(wq, w);
    ring_load<KS1, 1, false>(wq, w);
    if constexpr (RING > 3) ring_load<KS1, 2, false>(wq, w);
    if constexpr (RING > 4) ring_load<KS1, 3, false>(wq, w);
    if constexpr (RING > 5) ring_load<KS1, 4, false>(wq, w);
    {
        // biases -> LDS: [b1a | b1b] as 320 float4
        constexpr int NB = (NG_FLOATS / 4 + NTHR - 1) / NTHR;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int t = tid + NTHR * i;
            if (t < NG_FLOATS / 4) {
                const float* src = t < 256 ? p.b1a + 4 * t : p.b1b + 4 * (t - 256);
                *reinterpret_cast<float4*>(Bs + 4 * t) = *reinterpret_cast<const float4*>(src);
            }
        }
        Stage<4 * KS1> st;
        st.load(p.A1, 32 * KS1, nullptr, m0, M, tid);
        st.commit(Ah, Al, tid);
    }
    __syncthreads();
    const int n0 = wave * CT * 16 + 4 * fg;             // this lane's 4 output columns of column tile j start at n0 + 16 j
    f32x4_t accf[RT][CT];                               // P1 = position_encoder(A1), bias added at the end

    // ---- 1. P1 in four parts of 256 hidden columns
    zero_acc(accf);
    layer1<KS1, 0, false>(wq, a, w, Ah, Al, Hh, Hl, Bs + NG_1A, wave, fr, fg);
    steps<KS1, S::first_of(0) + KS1, 8, 0, false>(accf, wq, a, w, Hh, Hl, fr, fg);
    layer1<KS1, 1, false>(wq, a, w, Ah, Al, Hh, Hl, Bs + NG_1A + 256, wave, fr, fg);
    steps<KS1, S::first_of(1) + KS1, 8, 0, false>(accf, wq, a, w, Hh, Hl, fr, fg);
    layer1<KS1, 2, false>(wq, a, w, Ah, Al, Hh, Hl, Bs + NG_1A + 512, wave, fr, fg);
    steps<KS1, S::first_of(2) + KS1, 8, 0, false>(accf, wq, a, w, Hh, Hl, fr, fg);
    layer1<KS1, 3, false>(wq, a, w, Ah, Al, Hh, Hl, Bs + NG_1A + 768, wave, fr, fg);
    // read-back mapping of the output phase: lane -> (row r0 + 8 k, columns c4..c4+3 of 32); the row indices, the table rows and (row outputs) the
    // feature rows of the first 32 output columns travel under the last layer 2
    constexpr int NK = BM / 8;
    const int c4 = (lane & 7) * 4, r0 = lane >> 3;
    int ri[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int m = min(m0 + 8 * k + r0, M - 1);
        ri[k] = p.row_index ? p.row_index[m] : m;
    }
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
    steps<KS1, S::first_of(3) + KS1, 8, 0, false>(accf, wq, a, w, Hh, Hl, fr, fg);
    // ---- 2. pe = tab + (P1 + b); T path: Xk = pe + feat, Xv = feat as key16 hi + lo pairs.  Through a wave-private LDS tile
    // [BM rows][32 columns], then whole 128-byte row pieces (the output phase of the gated kernel).
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        const float4 fb = *reinterpret_cast<const float4*>(Bs + NG_1B + n0 + 16 * j);
#pragma unroll
        for (int i = 0; i < RT; ++i)
            accf[i][j] = f32x4_t{accf[i][j][0] + fb.x, accf[i][j][1] + fb.y, accf[i][j][2] + fb.z, accf[i][j][3] + fb.w};
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
                    make_float4(accf[i][2 * jp + j][0], accf[i][2 * jp + j][1], accf[i][2 * jp + j][2], accf[i][2 * jp + j][3]);
        __builtin_amdgcn_wave_barrier();               // the tile is read back by the same wave only
        const long long gcol = wave * CT * 16 + jp * 32 + c4;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int row = 8 * k + r0, m = m0 + row;
            float4 v = *reinterpret_cast<const float4*>(ot + row * OT_PITCH + c4);
            const float4 tv = tvq[k];
            v = make_float4(v.x + tv.x, v.y + tv.y, v.z + tv.z, v.w + tv.w);
            if (m < M) {
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
    }
}

constexpr int PX_BM = BM, PX_NTHR = NTHR;

}  // namespace
