// QueryGenerator shared conv: Conv2d(256, 256, 3, padding=1) + ReLU on the 7x7 RoI features, followed by AvgPool2d(7)
// (RH/utils/query_generator.py:298-304, 322-331, 352-358) -- conv + bias + ReLU + pooling fused, in two launches per call:
//   1. roi_conv_cell48_kernel: relu(conv + bias) of cell 48 of every RoI, 16 RoIs per MFMA row tile, left in the output buffer;
//   2. roi_conv_pool_kernel / roi_conv_pool_x3_kernel: one or two RoIs per block, cells 0..47 as THREE 16-row tiles per RoI; reads the
//      cell-48 term back from the output buffer, adds it where the fourth tile's row 0 used to be added, pools and overwrites the buffer.
// A RoI has 49 cells: as four row tiles of its own, a quarter of a block's MFMAs computed one row in sixteen.
//
// The implicit-GEMM route (gemm_bf16.hip, a_mode = 1) re-gathers every RoI row 9 times through L2 in 64x64 tiles, writes the
// [R*49, 256] fp32 conv output and needs a pooling launch.  Here the block keeps its RoI (49 cells x 256 channels key16 = 25 KB; cell 48
// stays: cells 40, 41 and 47 read it as a neighbour) in LDS once and every tap is just a remapped row index into it (out-of-range
// neighbours -> a zero row); the weights (256 x 2304 key16) are never staged: each wave streams the 64 output columns it owns as MFMA
// fragments straight from L2 through a register ring.  The weights are static, so they are stored FRAGMENT-MAJOR (mv2d_pack_wfrag_bf16:
// [k-step][column tile][lane][8]): a fragment load is one contiguous 1 KB per wave instead of 16 rows x 64 B (row-major fragment loads
// measured 74 us for this kernel: the TA walks 16 half-used lines per instruction and the L1 thrashes).  After the single staging barrier
// the waves run free -- no barrier, no LDS write in the 72-step k loop (fully unrolled so that hipcc keeps exact vmcnt counts for the
// ring).  The epilogue pools in registers + two shuffles and writes [R, 256] fp32: the 15 MB conv output and the avgpool launch disappear.
// k order = (tap, channel) like the implicit GEMM, so the conv sums are bit-identical; only the 49-term pooling sum is
// re-associated (fp32, ~1e-7).  Every output is bit for bit what the one-launch form with four row tiles per RoI wrote: each output element
// keeps its MFMA sequence and its single accumulator, and the pooling sum keeps its order (tests/test_gpu_conv_cell48.py).
#include "roiconv_walk.h"

namespace {

constexpr int CELLS = 49, KT = 9 * C;

// Keeps already requested loads where they were issued: the values count as used here, so hipcc cannot sink the loads to their first use
// in the epilogue (an exposed round trip there).
template <int A, int B>
__device__ __forceinline__ void pin_loaded(float (&v)[A][B]) {
#pragma unroll
    for (int a = 0; a < A; ++a)
#pragma unroll
        for (int b = 0; b < B; ++b) asm volatile("" : "+v"(v[a][b]));
}

// Cell 48 (the corner (6, 6)) of every RoI: out[r * ld_out + n] = relu(conv(cell 48) + bias), 16 RoIs per MFMA row tile (RoI r in row r % 16)
// instead of one row of a fourth tile per RoI in the pooling kernels below, which read the value back and add it as the last term of their
// fg = 0 lanes.  The block holds cells 40, 41, 47, 48 (the in-range neighbours of cell 48: taps 0, 1, 3, 4) of RB RoIs and a zero row (the
// other five taps) in LDS: RoI rl, neighbour c in row 4 rl + c, chunk slot ^ (rl & 15).  A wave owns ONE column tile and all RB / 16 row tiles;
// it runs the same 72 k-steps in the same (tap, channel) order on the same fragment-major weights with the same MFMA and one accumulator per
// output tile as the pooling kernels (zero taps included), so the value is bit for bit the one their fourth row tile held (an MFMA output
// element depends on its A row and B column only).  8 waves, grid (ceil(R / RB), 2): a block streams the weights of 128 columns (590 KB),
// the wave's 72 KB through a RING-deep register ring (nothing else hides the latency here: RB / 16 MFMAs per k-step).  RB = 64 RoIs fill the
// LDS (128 KB; 32 in split precision, two images): the launch reads 1.18 MB of weights per RB RoIs and the four cells once per 128 columns,
// 108 MB at R = 4800, which at the ~70 GB/s a CU draws from L2 is what its 14 us are made of.  Rows beyond R: clamped loads, no store.
template <bool X3, int RB>
__global__ __launch_bounds__(512) void roi_conv_cell48_kernel(const unsigned short* __restrict__ feat_hi, const unsigned short* __restrict__ feat_lo,
                                                              const unsigned short* __restrict__ Wh, const unsigned short* __restrict__ Wl,
                                                              const float* __restrict__ bias, float* __restrict__ out, int ld_out, int R) {
    constexpr int NT = RB / 16, NIMG = X3 ? 2 : 1, ZROW = RB * 4, RING = X3 ? 12 : 24;
    static_assert(72 % RING == 0, "compile-time ring slots");
    __shared__ __attribute__((aligned(16))) unsigned char xs[NIMG][(ZROW + 1) * C * 2];
    const int roi0 = blockIdx.x * RB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
    const int jt = blockIdx.y * 8 + wave;                 // the wave's column tile: columns 16 jt .. 16 jt + 15
    const long long w_off = ((long long)jt * 64 + lane) * 8;
    constexpr int KS_STRIDE = 16 * 64 * 8;
    Frag wqh[RING], wql[RING];
#pragma unroll
    for (int p = 0; p < RING - 1; ++p) {
        wqh[p].u = *reinterpret_cast<const uint4*>(Wh + w_off + p * KS_STRIDE);
        if (X3) wql[p].u = *reinterpret_cast<const uint4*>(Wl + w_off + p * KS_STRIDE);
    }
    const float b = bias[16 * jt + fr];
    {
        constexpr int NST = ZROW * 32 / 512;
        cv_u32x4 sh[NST], sl[NST];
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int c = tid + 512 * i, row = c >> 5, slot = c & 31, rl = row >> 2, nb = row & 3;
            const long long src = ((long long)min(roi0 + rl, R - 1) * CELLS + 40 + (nb & 1) + 7 * (nb >> 1)) * C + slot * 8;
            sh[i] = *reinterpret_cast<const cv_u32x4*>(feat_hi + src);
            if (X3) sl[i] = *reinterpret_cast<const cv_u32x4*>(feat_lo + src);
        }
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int c = tid + 512 * i, row = c >> 5, slot = c & 31, rl = row >> 2;
            const int dst = row * (C * 2) + ((slot ^ (rl & 15)) << 4);
            *reinterpret_cast<cv_u32x4*>(&xs[0][dst]) = sh[i];
            if (X3) *reinterpret_cast<cv_u32x4*>(&xs[NIMG - 1][dst]) = sl[i];
        }
        if (tid < 32)
#pragma unroll
            for (int m = 0; m < NIMG; ++m) *reinterpret_cast<cv_u32x4*>(&xs[m][ZROW * (C * 2) + (tid << 4)]) = cv_u32x4{0u, 0u, 0u, 0u};
    }
    f32x4_t acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    __syncthreads();

#pragma unroll
    for (int ks = 0; ks < 72; ++ks) {
        const int tap = ks >> 3, s = ks & 7;
        const int nb = tap == 0 ? 0 : tap == 1 ? 1 : tap == 3 ? 2 : tap == 4 ? 3 : -1;      // cells 40, 41, 47, 48; the other taps leave the RoI
        if (ks + RING - 1 < 72) {
            wqh[(ks + RING - 1) % RING].u = *reinterpret_cast<const uint4*>(Wh + w_off + (ks + RING - 1) * KS_STRIDE);
            if (X3) wql[(ks + RING - 1) % RING].u = *reinterpret_cast<const uint4*>(Wl + w_off + (ks + RING - 1) * KS_STRIDE);
        }
        __builtin_amdgcn_sched_barrier(0);
        Frag ah[NT], al[NT];
#pragma unroll
        for (int it = 0; it < NT; ++it) {
            const int off = nb < 0 ? ZROW * (C * 2) + ((4 * s + fg) << 4) : ((16 * it + fr) * 4 + nb) * (C * 2) + (((4 * s + fg) ^ fr) << 4);
            ah[it].u = *reinterpret_cast<const uint4*>(&xs[0][off]);
            if (X3) al[it].u = *reinterpret_cast<const uint4*>(&xs[NIMG - 1][off]);
        }
        if (X3) {                                        // per accumulator the order of roi_conv_pool_x3_kernel: lo x hi, hi x lo, hi x hi
#pragma unroll
            for (int it = 0; it < NT; ++it) acc[it] = mfma_k16_16x16x32(al[it].u, wqh[ks % RING].u, acc[it]);
#pragma unroll
            for (int it = 0; it < NT; ++it) acc[it] = mfma_k16_16x16x32(ah[it].u, wql[ks % RING].u, acc[it]);
        }
#pragma unroll
        for (int it = 0; it < NT; ++it) acc[it] = mfma_k16_16x16x32(ah[it].u, wqh[ks % RING].u, acc[it]);
    }
    // lane holds RoIs roi0 + 16 it + 4 fg + r of column 16 jt + fr
#pragma unroll
    for (int it = 0; it < NT; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int roi = roi0 + 16 * it + 4 * fg + r;
            if (roi < R) out[(long long)roi * ld_out + 16 * jt + fr] = relu_f(acc[it][r] + b);
        }
}

// NR RoIs per block: with NR = 2 the wave's weight fragments feed 6 instead of 3 row tiles (the 1.18 MB of conv weights stream through
// L2 / L1 once per block: 2.8 GB per 2400 RoIs at NR = 1).  Every RoI keeps its own three row tiles (LDS rows 50 rl .. 50 rl + 47 of the
// block, cell 48 and the zero row behind them), so the arithmetic per RoI — and the result, bit for bit — does not depend on NR or on
// which RoI it is paired with.
template <int NR>
__global__ __launch_bounds__(256, 2) void roi_conv_pool_kernel(const unsigned short* __restrict__ feat, const unsigned short* __restrict__ W,
                                                               const float* __restrict__ bias, float* __restrict__ out, int ld_out, int R) {
    // LDS rows: RoI rl at rows RS rl .. RS rl + 48, its zero row at RS rl + 49; the chunk swizzle goes by the row inside the RoI, so every
    // fragment address of RoI rl is that of RoI 0 plus a constant -> an instruction offset, no registers
    constexpr int RS = CELLS + 1, NROWS = RS * (NR - 1) + CELLS + 1, RING = NR == 1 ? 4 : 3, RT = 3 * NR;
    __shared__ __attribute__((aligned(16))) unsigned char xs[NROWS * C * 2];
    __shared__ float bs[C];
    const int roi0 = blockIdx.x * NR;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
    // ---- weight fragments of this wave's 64 output columns, register ring over the 72 k-steps (requested first: in flight while the RoIs are staged)
    // fragment-major weights: fragment (k-step ks, column tile jt) = 64 lanes x 16 B at ((ks * 16 + jt) * 64 + lane) * 8
    const unsigned short* w_src = W + ((long long)(wave * 4) * 64 + lane) * 8;
    constexpr int KS_STRIDE = 16 * 64 * 8, JT_STRIDE = 64 * 8;
    Frag wq[RING][4];
#pragma unroll
    for (int p = 0; p < RING - 1; ++p)
#pragma unroll
        for (int j = 0; j < 4; ++j) wq[p][j].u = *reinterpret_cast<const uint4*>(w_src + p * KS_STRIDE + j * JT_STRIDE);
    // ---- stage the RoIs: 16-byte chunks, chunk c of a RoI's row r at slot c ^ (r & 15).  All loads of a thread are issued before the first
    // LDS write (a rolled loop is one exposed memory round trip per iteration: 7 of them were a fifth of the block's time).
    {
        constexpr int NST = (NROWS * 32 + 255) / 256;
        cv_u32x4 st[NST];
        float bv = 0.f;
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int c = tid + 256 * i, row = c >> 5, slot = c & 31;
            const int rl = min(row / RS, NR - 1), cell = min(row - rl * RS, CELLS - 1);
            const bool ok = row - rl * RS < CELLS && roi0 + rl < R;
            st[i] = *reinterpret_cast<const cv_u32x4*>(feat + ((long long)min(roi0 + rl, R - 1) * CELLS + cell) * C + slot * 8);   // branch-free
            if (!ok) st[i] = cv_u32x4{0u, 0u, 0u, 0u};
        }
        bv = bias[tid];
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int c = tid + 256 * i, row = c >> 5, slot = c & 31;
            if (row < NROWS) *reinterpret_cast<cv_u32x4*>(xs + row * (C * 2) + ((slot ^ ((row - min(row / RS, NR - 1) * RS) & 15)) << 4)) = st[i];
        }
        bs[tid] = bv;                                    // the bias waits in LDS: a global load in the epilogue is another round trip
    }
    // cell coordinates of the 3 row tiles of a RoI for this lane (cell = 16 i + fr)
    int cy[3], cx[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { const int r = 16 * i + fr; cy[i] = r / 7; cx[i] = r - cy[i] * 7; }
    f32x4_t acc[RT][4];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float v48[NR][4];                                    // relu(conv + bias) of cell 48, left in out by roi_conv_cell48_kernel
    __syncthreads();
    // the three row-tile fragments of RoI rl at k-step ks: a tap is a remapped row index (out-of-range neighbours -> the zero row)
    auto load_a = [&](Frag (&a)[3], int ks, int rl) {
        const int tap = ks >> 3, s = ks & 7;
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            const int y = cy[it] + dy, x = cx[it] + dx;
            const bool ok = y >= 0 && y < 7 && x >= 0 && x < 7;
            const int src = ok ? y * 7 + x : CELLS;
            a[it].u = *reinterpret_cast<const uint4*>(xs + rl * (RS * C * 2) + src * (C * 2) + (((4 * s + fg) ^ (src & 15)) << 4));
        }
    };
    // the fragments are read one k-step ahead, a RoI's next ones in front of its current MFMAs: read in the step that uses them, every RoI
    // of every step opens with an LDS round trip that no MFMA of the wave covers (215 -> 210 us at 4800 RoIs)
    Frag an[NR][3];
#pragma unroll
    for (int rl = 0; rl < NR; ++rl) load_a(an[rl], 0, rl);

#pragma unroll
    for (int ks = 0; ks < 72; ++ks) {
        if (ks + RING - 1 < 72) {
#pragma unroll
            for (int j = 0; j < 4; ++j) wq[(ks + RING - 1) % RING][j].u = *reinterpret_cast<const uint4*>(w_src + (ks + RING - 1) * KS_STRIDE + j * JT_STRIDE);
        }
        // the first step without a prefetch: a ring slot's registers are free, and the last RING - 1 steps cover the round trip that the
        // epilogue would otherwise wait for
        if (ks + RING - 1 == 72) {
#pragma unroll
            for (int rl = 0; rl < NR; ++rl)
#pragma unroll
                for (int j = 0; j < 4; ++j) v48[rl][j] = out[(long long)min(roi0 + rl, R - 1) * ld_out + wave * 64 + 16 * j + fr];
        }
        __builtin_amdgcn_sched_barrier(0);           // keep the prefetch ahead (hipcc otherwise sinks the loads to their use)
#pragma unroll
        for (int rl = 0; rl < NR; ++rl) {               // one RoI's three row tiles at a time
            Frag a[3];
#pragma unroll
            for (int it = 0; it < 3; ++it) a[it] = an[rl][it];
            if (ks + 1 < 72) load_a(an[rl], ks + 1, rl);
#pragma unroll
            for (int it = 0; it < 3; ++it)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[3 * rl + it][j] = mfma_k16_16x16x32(a[it].u, wq[ks % RING][j].u, acc[3 * rl + it][j]);
        }
    }
    pin_loaded(v48);
    // ---- bias + ReLU + mean over the 49 cells: lane holds cells 16 i + 4 fg + r (< 48) of column 64 wave + 16 j + fr; cell 48 is the last
    // term of the fg = 0 lanes, as it was when it sat in row 0 of a fourth tile
#pragma unroll
    for (int rl = 0; rl < NR; ++rl) {
        if (roi0 + rl >= R) break;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = wave * 64 + 16 * j + fr;
            const float b = bs[n];
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) sum += relu_f(acc[3 * rl + i][j][r] + b);
            if (fg == 0) sum += v48[rl][j];
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            if (fg == 0) out[(long long)(roi0 + rl) * ld_out + n] = sum / 49.0f;
        }
    }
}

// Split-precision variant (index-exact route of the engine): the RoI cells come as key16 hi + lo pairs (mv2d_roi_align_ex: x ~ hi + lo), the
// weights as fragment-major key16 hi / lo copies (mv2d_split_key16 + mv2d_pack_wfrag_bf16); every product is a_lo w_hi + a_hi w_lo + a_hi w_hi
// (three MFMAs into one fp32 accumulator; the lo x lo term, 2^-18 relative, is dropped).  One RoI per block: two 25 KB LDS images, a
// 3-deep ring for both weight streams, the same tap remapping and epilogue as the bf16 kernel.  MFMA-bound (3 x 2304 MFMAs per wave
// against 2.4 MB of weight fragments per block).
__global__ __launch_bounds__(256, 2) void roi_conv_pool_x3_kernel(const unsigned short* __restrict__ feat_hi, const unsigned short* __restrict__ feat_lo,
                                                                  const unsigned short* __restrict__ Wh, const unsigned short* __restrict__ Wl,
                                                                  const float* __restrict__ bias, float* __restrict__ out, int ld_out, int R) {
    constexpr int NROWS = CELLS + 1, RING = 3;
    __shared__ __attribute__((aligned(16))) unsigned char xh[NROWS * C * 2], xl[NROWS * C * 2];
    __shared__ float bs[C];
    const int roi = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
    const long long w_off = ((long long)(wave * 4) * 64 + lane) * 8;
    constexpr int KS_STRIDE = 16 * 64 * 8, JT_STRIDE = 64 * 8;
    Frag wqh[RING][4], wql[RING][4];
#pragma unroll
    for (int p = 0; p < RING - 1; ++p)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            wqh[p][j].u = *reinterpret_cast<const uint4*>(Wh + w_off + p * KS_STRIDE + j * JT_STRIDE);
            wql[p][j].u = *reinterpret_cast<const uint4*>(Wl + w_off + p * KS_STRIDE + j * JT_STRIDE);
        }
    {
        constexpr int NST = (NROWS * 32 + 255) / 256;
        cv_u32x4 sh[NST], sl[NST];
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int c = tid + 256 * i, row = c >> 5, slot = c & 31;
            const bool ok = row < CELLS;
            const long long src = ((long long)roi * CELLS + min(row, CELLS - 1)) * C + slot * 8;
            sh[i] = *reinterpret_cast<const cv_u32x4*>(feat_hi + src);
            sl[i] = *reinterpret_cast<const cv_u32x4*>(feat_lo + src);
            if (!ok) { sh[i] = cv_u32x4{0u, 0u, 0u, 0u}; sl[i] = cv_u32x4{0u, 0u, 0u, 0u}; }
        }
        const float bv = bias[tid];
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int c = tid + 256 * i, row = c >> 5, slot = c & 31;
            if (row < NROWS) {
                *reinterpret_cast<cv_u32x4*>(xh + row * (C * 2) + ((slot ^ (row & 15)) << 4)) = sh[i];
                *reinterpret_cast<cv_u32x4*>(xl + row * (C * 2) + ((slot ^ (row & 15)) << 4)) = sl[i];
            }
        }
        bs[tid] = bv;
    }
    int cy[3], cx[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { const int r = 16 * i + fr; cy[i] = r / 7; cx[i] = r - cy[i] * 7; }
    f32x4_t acc[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float v48[1][4];                                     // cell 48's term from roi_conv_cell48_kernel<true>, as in roi_conv_pool_kernel
    __syncthreads();

#pragma unroll
    for (int ks = 0; ks < 72; ++ks) {
        const int tap = ks >> 3, s = ks & 7;
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
        if (ks + RING - 1 < 72) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                wqh[(ks + RING - 1) % RING][j].u = *reinterpret_cast<const uint4*>(Wh + w_off + (ks + RING - 1) * KS_STRIDE + j * JT_STRIDE);
                wql[(ks + RING - 1) % RING][j].u = *reinterpret_cast<const uint4*>(Wl + w_off + (ks + RING - 1) * KS_STRIDE + j * JT_STRIDE);
            }
        }
        if (ks + RING - 1 == 72) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v48[0][j] = out[(long long)roi * ld_out + wave * 64 + 16 * j + fr];
        }
        __builtin_amdgcn_sched_barrier(0);
        Frag ah[3], al[3];
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            const int y = cy[it] + dy, x = cx[it] + dx;
            const bool ok = y >= 0 && y < 7 && x >= 0 && x < 7;
            const int src = ok ? y * 7 + x : CELLS;
            const int off = src * (C * 2) + (((4 * s + fg) ^ (src & 15)) << 4);
            ah[it].u = *reinterpret_cast<const uint4*>(xh + off);
            al[it].u = *reinterpret_cast<const uint4*>(xl + off);
        }
#pragma unroll
        for (int it = 0; it < 3; ++it)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[it][j] = mfma_k16_16x16x32(al[it].u, wqh[ks % RING][j].u, acc[it][j]);
#pragma unroll
        for (int it = 0; it < 3; ++it)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[it][j] = mfma_k16_16x16x32(ah[it].u, wql[ks % RING][j].u, acc[it][j]);
#pragma unroll
        for (int it = 0; it < 3; ++it)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[it][j] = mfma_k16_16x16x32(ah[it].u, wqh[ks % RING][j].u, acc[it][j]);
    }
    pin_loaded(v48);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = wave * 64 + 16 * j + fr;
        const float b = bs[n];
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) sum += relu_f(acc[i][j][r] + b);
        if (fg == 0) sum += v48[0][j];
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        if (fg == 0) out[(long long)roi * ld_out + n] = sum / 49.0f;
    }
}

// Any RoI size s x s, 1 <= s <= 14 (the 7 x 7 kernels above stay the shipped instances): the chunked window walk of roiconv_walk.inc, one RoI per
// block; every chunk adds bias + ReLU of its cells to the per-column sums, which are pooled behind the last one.
// X3: the split-precision products of roi_conv_pool_x3_kernel; otherwise key16 x key16.
template <bool X3>
__global__ __launch_bounds__(256, X3 ? 1 : 2) void roi_conv_pool_s_kernel(const unsigned short* __restrict__ feat_hi, const unsigned short* __restrict__ feat_lo,
                                                                         const unsigned short* __restrict__ Wh, const unsigned short* __restrict__ Wl,
                                                                         const float* __restrict__ bias, float* __restrict__ out, int ld_out, int R, int s) {
    float psum[4] = {0.f, 0.f, 0.f, 0.f};
#define ROI_CONV_WALK_CELL(v, cell, n, j) psum[j] += (v)
#include "roiconv_walk.inc"
#undef ROI_CONV_WALK_CELL
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float sum = psum[j];
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        if (fg == 0) out[(long long)roi * ld_out + wave * 64 + 16 * j + fr] = sum / (float)S2;
    }
}

// row-major W [N, K] bf16 -> fragment-major Wp[K/32][N/16][64][8]: Wp[ks][jt][fr + 16 fg][e] = W[16 jt + fr][32 ks + 8 fg + e]
__global__ void pack_wfrag_kernel(const unsigned short* __restrict__ W, unsigned short* __restrict__ Wp, int N, int K) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;          // one 16-byte chunk per thread
    const long long total = (long long)N * K / 8;
    if (idx >= total) return;
    const int lane = idx & 63;
    const long long t = idx >> 6;
    const int jt = (int)(t % (N / 16)), ks = (int)(t / (N / 16));
    const int fr = lane & 15, fg = lane >> 4;
    *reinterpret_cast<uint4*>(Wp + idx * 8) = *reinterpret_cast<const uint4*>(W + (long long)(16 * jt + fr) * K + 32 * ks + 8 * fg);
}

}  // namespace

extern "C" int mv2d_pack_wfrag_bf16(const void* W, void* Wp, int N, int K, void* stream) {
    MV2D_CHECK_ARG(W && Wp && N > 0 && K > 0 && (N % 16) == 0 && (K % 32) == 0, "mv2d_pack_wfrag_bf16: N % 16 == 0 and K % 32 == 0 required");
    const long long total = (long long)N * K / 8;
    hipLaunchKernelGGL(pack_wfrag_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned short*)W, (unsigned short*)Wp, N, K);
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}

namespace {

// the argument check of the key16 entries, with or without a RoI size
int check_pool_args(const void* roi_feat, const void* W, const float* bias, const float* out, int ld_out) {
    MV2D_CHECK_ARG(roi_feat && W && bias && out && ld_out >= C, "mv2d_qg_conv_pool: bad args");
    MV2D_CHECK_ARG(((uintptr_t)roi_feat & 15) == 0 && ((uintptr_t)W & 15) == 0, "mv2d_qg_conv_pool: operands must be 16-byte aligned");
    return MV2D_OK;
}

// ... and of the split-precision entries
int check_pool_x3_args(const void* roi_feat_hi, const void* roi_feat_lo, const void* W_hi, const void* W_lo, const float* bias, const float* out, int ld_out) {
    MV2D_CHECK_ARG(roi_feat_hi && roi_feat_lo && W_hi && W_lo && bias && out && ld_out >= C, "mv2d_qg_conv_pool_x3: bad args");
    MV2D_CHECK_ARG(((uintptr_t)roi_feat_hi & 15) == 0 && ((uintptr_t)roi_feat_lo & 15) == 0 && ((uintptr_t)W_hi & 15) == 0 && ((uintptr_t)W_lo & 15) == 0,
                   "mv2d_qg_conv_pool_x3: operands must be 16-byte aligned");
    return MV2D_OK;
}

}  // namespace

extern "C" int mv2d_qg_conv_pool(const void* roi_feat, const void* W, const float* bias, float* out, int ld_out, int R, void* stream) {
    if (const int rc = check_pool_args(roi_feat, W, bias, out, ld_out)) return rc;
    if (R == 0) return MV2D_OK;
    // cell 48 of every RoI first (its term travels in out), then the pooling kernel on the other 48 cells
    hipLaunchKernelGGL((roi_conv_cell48_kernel<false, 64>), dim3(cdiv(R, 64), 2), dim3(512), 0, (hipStream_t)stream, (const unsigned short*)roi_feat,
                       nullptr, (const unsigned short*)W, nullptr, bias, out, ld_out, R);
    MV2D_LAUNCH_CHECK();
    // two RoIs per block once the grid fills the chip either way (identical results, see the kernel)
    const int nr = R >= 1024 ? 2 : 1;
    if (nr == 2)
        hipLaunchKernelGGL(roi_conv_pool_kernel<2>, dim3(cdiv(R, 2)), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)roi_feat,
                           (const unsigned short*)W, bias, out, ld_out, R);
    else
        hipLaunchKernelGGL(roi_conv_pool_kernel<1>, dim3(R), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)roi_feat,
                           (const unsigned short*)W, bias, out, ld_out, R);
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}

extern "C" int mv2d_qg_conv_pool_x3(const void* roi_feat_hi, const void* roi_feat_lo, const void* W_hi, const void* W_lo, const float* bias, float* out,
                                    int ld_out, int R, void* stream) {
    if (const int rc = check_pool_x3_args(roi_feat_hi, roi_feat_lo, W_hi, W_lo, bias, out, ld_out)) return rc;
    if (R == 0) return MV2D_OK;
    hipLaunchKernelGGL((roi_conv_cell48_kernel<true, 32>), dim3(cdiv(R, 32), 2), dim3(512), 0, (hipStream_t)stream, (const unsigned short*)roi_feat_hi,
                       (const unsigned short*)roi_feat_lo, (const unsigned short*)W_hi, (const unsigned short*)W_lo, bias, out, ld_out, R);
    MV2D_LAUNCH_CHECK();
    hipLaunchKernelGGL(roi_conv_pool_x3_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)roi_feat_hi,
                       (const unsigned short*)roi_feat_lo, (const unsigned short*)W_hi, (const unsigned short*)W_lo, bias, out, ld_out, R);
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}

// s x s cells per RoI, 1 <= s <= 14: the 7 x 7 kernels for s = 7, roi_conv_pool_s_kernel otherwise
extern "C" int mv2d_qg_conv_pool_s(const void* roi_feat, const void* W, const float* bias, float* out, int ld_out, int R, int roi_size, void* stream) {
    MV2D_CHECK_ARG(roi_size >= 1 && roi_size <= 14, "mv2d_qg_conv_pool_s: roi_size must be in [1, 14]");
    if (roi_size == 7) return mv2d_qg_conv_pool(roi_feat, W, bias, out, ld_out, R, stream);
    if (const int rc = check_pool_args(roi_feat, W, bias, out, ld_out)) return rc;
    if (R == 0) return MV2D_OK;
    hipLaunchKernelGGL(roi_conv_pool_s_kernel<false>, dim3(R), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)roi_feat, nullptr,
                       (const unsigned short*)W, nullptr, bias, out, ld_out, R, roi_size);
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}

extern "C" int mv2d_qg_conv_pool_x3_s(const void* roi_feat_hi, const void* roi_feat_lo, const void* W_hi, const void* W_lo, const float* bias, float* out,
                                      int ld_out, int R, int roi_size, void* stream) {
    MV2D_CHECK_ARG(roi_size >= 1 && roi_size <= 14, "mv2d_qg_conv_pool_x3_s: roi_size must be in [1, 14]");
    if (roi_size == 7) return mv2d_qg_conv_pool_x3(roi_feat_hi, roi_feat_lo, W_hi, W_lo, bias, out, ld_out, R, stream);
    if (const int rc = check_pool_x3_args(roi_feat_hi, roi_feat_lo, W_hi, W_lo, bias, out, ld_out)) return rc;
    if (R == 0) return MV2D_OK;
    hipLaunchKernelGGL(roi_conv_pool_s_kernel<true>, dim3(R), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)roi_feat_hi,
                       (const unsigned short*)roi_feat_lo, (const unsigned short*)W_hi, (const unsigned short*)W_lo, bias, out, ld_out, R, roi_size);
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}
