// The query generator's MLP tail + the query positional embedding as ONE launch (mv2d_qg_tail_x3):
//   enc[:, :1024] = clamp(ReLU(shared_fcs.0(x2)), 5e3)      (RH/utils/query_generator.py:359-381)
//   enc1 = ReLU(extra_enc.0([enc | intrinsics]))             (the 32 intrinsics columns are read from enc[:, 1024:1056])
//   enc2 = ReLU(extra_enc.2(enc1))
//   center, xyz, ref, posemb, qpos as query_embed_fused_x3_kernel (rowblock.hip)
// BITWISE the four launches it replaces (3 x linear_x3_kernel + query_embed_fused_x3_kernel): every output element keeps its two
// accumulators (a0 += x_hi.w_hi; a1 += x_lo.w_hi; a1 += x_hi.w_lo per k-step, k ascending), (a0 + a1) + b, ReLU, clamp, and the hi / lo
// split of exactly the fp32 value the chain stores between its launches.  The hidden layers never leave the CU.
//
// Block = 32 rows (2 MFMA row tiles), 8 waves.  Every layer: wave w owns NCT adjacent 16-column tiles for both row tiles, i.e. 2 NCT
// independent (a0, a1) chain pairs; within a k-step all a0 MFMAs are issued before the a1 ones, so dependent MFMAs are >= 2 NCT apart.
// Weights go L2 -> registers through ONE 4-slot ring that runs across all layers: at k-step s of a phase the fragments of stream position
// s + 3 are requested -- the next phase's first three k-steps during the last three of this one -- so no phase starts with a cold weight load.
// Activation fragments are read from the LDS images one k-step ahead of their MFMAs.
// The fc layer is produced in 4 parts of 256 hidden columns (hi / lo images, double buffered) and each part is consumed as one K chunk
// of extra_enc.0 while the next part is computed: one barrier per part.
// A launch of 64 or more compute blocks adds 64 blocks that only read the weights into the L2s ahead of them (warm_l2 below).
//
// LDS (100 KB, regions alias once their readers have passed a barrier):
//   [  0, 32K) x2 images (pitch 512)            -> [0, 64K) enc1 images (pitch 1024) -> [0, 64K) posemb images (pitch 1024)
//   [ 32, 96K) fc part images, 2 x (hi | lo)    -> [64K, 64K + 33280) enc2 fp32 (pitch 260 floats) -> [64K, 96K) hidden images of query_embedding
//   [ 96,100K) intrinsics images (pitch 64)
#include "x3_tile.h"

namespace {

struct QgTailParams {
    const float* x2; const float* enc; int ld_enc;
    const uint4* fch; const uint4* fcl; const float* fcb;
    const uint4* e0h; const uint4* e0l; const float* e0b;
    const uint4* e2h; const uint4* e2l; const float* e2b;
    const float* Wc; const float* bc; const float* minv; const float* dim_t;
    float pc0, pc1, pc2, pd0, pd1, pd2;
    const uint4* q0h; const uint4* q0l; const float* q0b;
    const uint4* q2h; const uint4* q2l; const float* q2b;
    float* center; float* xyz; float* ref; float* posemb; float* qpos; int R;
    int nwork;                                          // blocks 0 .. nwork - 1 compute; the rest warm the L2 (warm_l2)
};

constexpr int RT = 2;                                   // row tiles per block
constexpr int RD = 4;                                   // ring slots: the requests run RD - 1 k-steps ahead of the MFMAs
struct Ring { BFrag h[RD][4], l[RD][4]; };              // RD k-steps x up to 4 column tiles x (hi, lo)
// fragment-major weights [K/32][ntile][lane][8 x 16 bit] as uint4 per lane; tile0 = this wave's first column tile (wave-uniform)
struct WSrc { const uint4* h; const uint4* l; int ntile; int tile0; };

// (fragment address = wave-uniform base + 16 * lane: scalar address arithmetic, one VGPR of offsets for the whole weight stream)
template <int NCT>
__device__ __forceinline__ void ring_load(Ring& rg, int slot, const WSrc& w, int ks, unsigned lane16) {
#pragma unroll
    for (int j = 0; j < NCT; ++j) {
        const int idx = (ks * w.ntile + w.tile0 + j) << 6;
        rg.h[slot][j].u = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(w.h + idx) + lane16);
        rg.l[slot][j].u = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(w.l + idx) + lane16);
    }
}

template <int NCT>
__device__ __forceinline__ void zero_acc(f32x4_t (&a0)[NCT][RT], f32x4_t (&a1)[NCT][RT]) {
#pragma unroll
    for (int j = 0; j < NCT; ++j)
#pragma unroll
        for (int t = 0; t < RT; ++t) { a0[j][t] = f32x4_t{0.f, 0.f, 0.f, 0.f}; a1[j][t] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
}

// NK k-steps of one layer.  BASE = ring slot of this phase's k-step 0 (its first RD - 1 k-steps are already requested); the last RD - 1 k-steps
// request the first RD - 1 of the next phase (NCT_NEXT column tiles of `wn` from k-step ksn0; NCT_NEXT = 0: nothing follows).
// xfrag(s, xh, xl): the activation fragments (hi, lo) of both row tiles for k-step s.
template <int NCT, int NK, int BASE, int NCT_NEXT, class XF>
__device__ __forceinline__ void phase(f32x4_t (&a0)[NCT][RT], f32x4_t (&a1)[NCT][RT], Ring& rg, const WSrc& w, int ks0, const WSrc& wn, int ksn0,
                                      unsigned lane16, XF xfrag) {
    static_assert(NK >= RD - 1, "the last RD - 1 k-steps of a phase request the first RD - 1 of the next");
    BFrag xh[2][RT], xl[2][RT];
    xfrag(0, xh[0], xl[0]);
#pragma unroll
    for (int s = 0; s < NK; ++s) {
        constexpr int A = RD - 1;
        if (s + A < NK) ring_load<NCT>(rg, (BASE + s + A) % RD, w, ks0 + s + A, lane16);
        else if (NCT_NEXT > 0) ring_load<(NCT_NEXT > 0 ? NCT_NEXT : 1)>(rg, (BASE + s + A) % RD, wn, ksn0 + s + A - NK, lane16);
        if (s + 1 < NK) xfrag(s + 1, xh[(s + 1) & 1], xl[(s + 1) & 1]);
        const int slot = (BASE + s) % RD, xb = s & 1;
#pragma unroll
        for (int j = 0; j < NCT; ++j)
#pragma unroll
            for (int t = 0; t < RT; ++t) a0[j][t] = mfma_q16_16x16x32(xh[xb][t].v, rg.h[slot][j].v, a0[j][t], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < NCT; ++j)
#pragma unroll
            for (int t = 0; t < RT; ++t) a1[j][t] = mfma_q16_16x16x32(xl[xb][t].v, rg.h[slot][j].v, a1[j][t], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < NCT; ++j)
#pragma unroll
            for (int t = 0; t < RT; ++t) a1[j][t] = mfma_q16_16x16x32(xh[xb][t].v, rg.l[slot][j].v, a1[j][t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);               // keep the requests where they are: hoisted further, the ring no longer fits the register file
    }
}

// element (row, col) of a pair of 16-bit images with `pitch` bytes per row: 16-byte chunk c of row r at c ^ (r & 15)
__device__ __forceinline__ void put_q16(unsigned char* ih, unsigned char* il, int pitch, int row, int col, float v) {
    unsigned short hi, lo;
    split_q16(v, hi, lo);
    const int off = row * pitch + (((col >> 3) ^ (row & 15)) << 4) + (col & 7) * 2;
    *reinterpret_cast<unsigned short*>(ih + off) = hi;
    *reinterpret_cast<unsigned short*>(il + off) = lo;
}

// An opaque copy of a lane index: what a stage derives from it (LDS offsets, output addresses) is then computed in that stage instead of being
// hoisted to the top of the kernel and carried -- spilled -- through the phases that need every register for the ring and the accumulators.
__device__ __forceinline__ int fresh(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

constexpr int LDS_X2H = 0, LDS_X2L = 16384;
constexpr int LDS_PART = 32768;                         // part buffer b: hi at LDS_PART + b * 32768, lo 16384 behind
constexpr int LDS_INTR = 98304;                         // hi [32][64 B], lo 2048 behind
constexpr int LDS_E1H = 0, LDS_E1L = 32768;             // enc1 / posemb images, pitch 1024
constexpr int LDS_E2F = 65536, E2_PITCH = 260;          // enc2 fp32, pitch 260 floats
constexpr int LDS_HH = 65536, LDS_HL = 81920;           // hidden images of query_embedding, pitch 512
constexpr int LDS_BYTES = 102400;

// Helper blocks of a large launch.  In a frame the 4.4 MB of weights are cold when this kernel starts (the stages in front of it have
// pushed them out of the 4 MB L2s), and a compute block, which streams them through three k-steps of requests, then waits on memory
// latency: 69 us per 4800 rows against 54 us with warm L2s.  The launch leaves 100 of the 256 CUs idle, so 8 extra blocks per XCD (the
// dispatcher deals consecutive blocks round robin to the XCDs, common.h) read every weight once, in the order the compute blocks use
// them and with 16 requests per lane in flight; the values are dropped.  Speed only: nothing depends on what a helper has read.
__device__ __forceinline__ void warm_l2(const QgTailParams& p, int rank, int per_xcd, int tid) {
    const uint4* arr[10] = {p.fch, p.fcl, p.e0h, p.e0l, p.e2h, p.e2l, p.q0h, p.q0l, p.q2h, p.q2l};
    const int n512[10] = {64, 64, 132, 132, 32, 32, 24, 24, 16, 16};              // uint4 per array / 512: [N,K] 16-bit = N K / 4096
#pragma unroll 1
    for (int a = 0; a < 10; ++a) {
        const uint4* w = arr[a] + tid;
#pragma unroll 1
        for (int i0 = rank; i0 < n512[a]; i0 += 16 * per_xcd) {
            uint4 v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int i = i0 + u * per_xcd;
                if (i < n512[a]) v[u] = w[i * 512];
                else v[u] = make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) asm volatile("" ::"v"(v[u].x), "v"(v[u].y), "v"(v[u].z), "v"(v[u].w));
        }
    }
}

__global__ __launch_bounds__(512) void qg_tail_x3_kernel(QgTailParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    if ((int)blockIdx.x >= p.nwork) {                    // (block-uniform, before any barrier)
        warm_l2(p, ((int)blockIdx.x - p.nwork) >> 3, ((int)gridDim.x - p.nwork) >> 3, threadIdx.x);
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * 32;
    const unsigned lane16 = lane * 16;

    // ---- x2 tile and the intrinsics columns (rows >= R read row R - 1: the chain's clamp), first weight fragments behind them
    float4 ar[4], ai;
    {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 512 * i, row = idx >> 6, q = idx & 63;
            ar[i] = *reinterpret_cast<const float4*>(p.x2 + (long long)min(m0 + row, p.R - 1) * 256 + 4 * q);
        }
        const int row = (tid & 255) >> 3, q = tid & 7;
        ai = *reinterpret_cast<const float4*>(p.enc + (long long)min(m0 + row, p.R - 1) * p.ld_enc + 1024 + 4 * q);
    }
    const WSrc w_e0{p.e0h, p.e0l, 32, 4 * wave}, w_e2{p.e2h, p.e2l, 16, 2 * wave};
    const WSrc w_q0{p.q0h, p.q0l, 16, 2 * wave}, w_q2{p.q2h, p.q2l, 16, 2 * wave};
    auto w_fc = [&](int part) { return WSrc{p.fch, p.fcl, 64, 16 * part + 2 * wave}; };
    Ring rg;
#pragma unroll
    for (int s = 0; s < RD - 1; ++s) ring_load<2>(rg, s, w_fc(0), s, lane16);
    {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 512 * i, row = idx >> 6, q = idx & 63;
            const int off = row * 512 + (((q >> 1) ^ (row & 15)) << 4) + (q & 1) * 8;
            uint2 hi, lo;
            split4(ar[i], hi, lo);
            *reinterpret_cast<uint2*>(lds + LDS_X2H + off) = hi;
            *reinterpret_cast<uint2*>(lds + LDS_X2L + off) = lo;
        }
        if (tid < 256) {
            const int row = tid >> 3, q = tid & 7;
            uint2 hi, lo;
            split4(ai, hi, lo);
            *reinterpret_cast<uint2*>(lds + LDS_INTR + row * 64 + q * 8) = hi;
            *reinterpret_cast<uint2*>(lds + LDS_INTR + 2048 + row * 64 + q * 8) = lo;
        }
    }
    __syncthreads();

    // activation fragments of k-step s from images with 512 B rows (hi at `base`, lo `lo_off` behind) / 1024 B rows
    auto x512 = [&](int base, int lo_off) {
        const int fr = fresh(lane) & 15, fg = fresh(lane) >> 4;
        return [=](int s, BFrag (&xh)[RT], BFrag (&xl)[RT]) {
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                const int off = base + t * 8192 + fr * 512 + (((4 * s + fg) ^ fr) << 4);
                xh[t].u = *reinterpret_cast<const uint4*>(lds + off);
                xl[t].u = *reinterpret_cast<const uint4*>(lds + off + lo_off);
            }
        };
    };
    auto x1024 = [&]() {
        const int fr = fresh(lane) & 15, fg = fresh(lane) >> 4;
        return [=](int s, BFrag (&xh)[RT], BFrag (&xl)[RT]) {
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                const int off = LDS_E1H + (16 * t + fr) * 1024 + (((4 * s + fg) ^ fr) << 4);
                xh[t].u = *reinterpret_cast<const uint4*>(lds + off);
                xl[t].u = *reinterpret_cast<const uint4*>(lds + off + (LDS_E1L - LDS_E1H));
            }
        };
    };
    auto x_x2 = [&]() { return x512(LDS_X2H, LDS_X2L - LDS_X2H); };
    // the biases of a wave's column tiles, requested BEFORE the phase whose epilogue adds them: waiting for them then leaves the ring's
    // younger requests in flight (a load issued in the epilogue would have to drain the ring first)
    auto load_bias2 = [&](float (&b)[2], const float* bias) {
        const int fr = fresh(lane) & 15;
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = bias[(2 * wave + j) * 16 + fr];
    };
    // bias + ReLU + clamp 5e3 + split of fc part `part` into part buffer `part & 1`
    auto fc_out = [&](int part, f32x4_t (&a0)[2][RT], f32x4_t (&a1)[2][RT], const float (&bias)[2]) {
        unsigned char* ih = lds + LDS_PART + (part & 1) * 32768;
        const int fr = fresh(lane) & 15, fg = fresh(lane) >> 4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int lc = (2 * wave + j) * 16 + fr;
            const float b = bias[j];
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = relu_f((a0[j][t][r] + a1[j][t][r]) + b);
                    v = fminf(fmaxf(v, -5e3f), 5e3f);
                    put_q16(ih, ih + 16384, 512, 16 * t + 4 * fg + r, lc, v);
                }
        }
    };

    // ring slot of every phase's first k-step: the stream positions run on across the phases
    constexpr int B_FC0 = 0, B_FC1 = (B_FC0 + 8) % RD, B_E0C0 = (B_FC1 + 8) % RD, B_FC2 = (B_E0C0 + 8) % RD, B_E0C1 = (B_FC2 + 8) % RD;
    constexpr int B_FC3 = (B_E0C1 + 8) % RD, B_E0C2 = (B_FC3 + 8) % RD, B_E0C3 = (B_E0C2 + 8) % RD, B_E2 = (B_E0C3 + 9) % RD;
    constexpr int B_Q0 = (B_E2 + 16) % RD, B_Q2 = (B_Q0 + 12) % RD;

    f32x4_t e0a0[4][RT], e0a1[4][RT];                    // extra_enc.0: 4 column tiles per wave, accumulated over the 4 parts + intrinsics
    zero_acc<4>(e0a0, e0a1);
    {
        f32x4_t a0[2][RT], a1[2][RT];
        float bv[2];
        // ---- fc part 0
        load_bias2(bv, p.fcb);
        zero_acc<2>(a0, a1);
        phase<2, 8, B_FC0, 2>(a0, a1, rg, w_fc(0), 0, w_fc(1), 0, lane16, x_x2());
        fc_out(0, a0, a1, bv);
        __syncthreads();
        // ---- fc part 1 | extra_enc.0 chunk 0
        load_bias2(bv, p.fcb + 256);
        zero_acc<2>(a0, a1);
        phase<2, 8, B_FC1, 4>(a0, a1, rg, w_fc(1), 0, w_e0, 0, lane16, x_x2());
        fc_out(1, a0, a1, bv);
        phase<4, 8, B_E0C0, 2>(e0a0, e0a1, rg, w_e0, 0, w_fc(2), 0, lane16, x512(LDS_PART, 16384));
        __syncthreads();
        // ---- fc part 2 | chunk 1
        load_bias2(bv, p.fcb + 512);
        zero_acc<2>(a0, a1);
        phase<2, 8, B_FC2, 4>(a0, a1, rg, w_fc(2), 0, w_e0, 8, lane16, x_x2());
        fc_out(2, a0, a1, bv);
        phase<4, 8, B_E0C1, 2>(e0a0, e0a1, rg, w_e0, 8, w_fc(3), 0, lane16, x512(LDS_PART + 32768, 16384));
        __syncthreads();
        // ---- fc part 3 | chunk 2
        load_bias2(bv, p.fcb + 768);
        zero_acc<2>(a0, a1);
        phase<2, 8, B_FC3, 4>(a0, a1, rg, w_fc(3), 0, w_e0, 16, lane16, x_x2());
        fc_out(3, a0, a1, bv);
        phase<4, 8, B_E0C2, 4>(e0a0, e0a1, rg, w_e0, 16, w_e0, 24, lane16, x512(LDS_PART, 16384));
        __syncthreads();
    }
    // ---- chunk 3 + the intrinsics k-step (k-step 32 of extra_enc.0, the last one)
    float be0[4];
    {
        const int fr = fresh(lane) & 15;
#pragma unroll
        for (int j = 0; j < 4; ++j) be0[j] = p.e0b[(4 * wave + j) * 16 + fr];
    }
    {
        const auto x_p1 = x512(LDS_PART + 32768, 16384);
        const int fr = fresh(lane) & 15, fg = fresh(lane) >> 4;
        phase<4, 9, B_E0C3, 2>(e0a0, e0a1, rg, w_e0, 24, w_e2, 0, lane16, [&](int s, BFrag (&xh)[RT], BFrag (&xl)[RT]) {
            if (s < 8) { x_p1(s, xh, xl); return; }
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                const int off = LDS_INTR + (16 * t + fr) * 64 + fg * 16;
                xh[t].u = *reinterpret_cast<const uint4*>(lds + off);
                xl[t].u = *reinterpret_cast<const uint4*>(lds + off + 2048);
            }
        });
    }
    __syncthreads();                                     // every reader of the x2 / part images is done: enc1 takes their place
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int fr = fresh(lane) & 15, fg = fresh(lane) >> 4;
        const int col = (4 * wave + j) * 16 + fr;
        const float b = be0[j];
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                put_q16(lds + LDS_E1H, lds + LDS_E1L, 1024, 16 * t + 4 * fg + r, col, relu_f((e0a0[j][t][r] + e0a1[j][t][r]) + b));
    }
    __syncthreads();
    f32x4_t a0[2][RT], a1[2][RT];
    float bv[2];
    // what the row stage behind extra_enc.2 reads from memory, requested before that layer's k-steps (one exposed latency less per row)
    // (channel = 128 axis + 2 lane + (j & 1): a wave evaluates sinf for all its lanes, then cosf, instead of both for every channel;
    //  dim_t depends on the channel within the axis only, i.e. on (lane, j & 1))
    const int lane_c = fresh(tid) & 63;
    float4 wc[3];
    float bcv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { wc[k] = *reinterpret_cast<const float4*>(p.Wc + k * C + lane_c * 4); bcv[k] = p.bc[k]; }
    const float2 dt = *reinterpret_cast<const float2*>(p.dim_t + 2 * lane_c);
    // lidar2img inverse of this wave's 4 RoIs: lane 16 i + k holds element k of row i (read back with readlane)
    const float mi = p.minv[min(m0 + 4 * wave + (lane_c >> 4), p.R - 1) * 16 + (lane_c & 15)];
    // ---- extra_enc.2 -> enc2 (fp32 tile: fc_center reads it unrounded)
    load_bias2(bv, p.e2b);
    zero_acc<2>(a0, a1);
    phase<2, 16, B_E2, 2>(a0, a1, rg, w_e2, 0, w_q0, 0, lane16, x1024());
    {
        float* e2f = reinterpret_cast<float*>(lds + LDS_E2F);
        const int fr = fresh(lane) & 15, fg = fresh(lane) >> 4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = (2 * wave + j) * 16 + fr;
            const float b = bv[j];
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) e2f[(16 * t + 4 * fg + r) * E2_PITCH + col] = relu_f((a0[j][t][r] + a1[j][t][r]) + b);
        }
    }
    __syncthreads();
    // ---- fc_center, center2lidar, normalisation, pos2posemb3d: wave w finishes rows 4 w .. 4 w + 3 (operation order of query_embed_fused_x3_kernel)
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        const int lane = lane_c;
        const int row = 4 * wave + i;
        const int r = min(m0 + row, p.R - 1);
        const bool live = m0 + row < p.R;
        const float4 e = *reinterpret_cast<const float4*>(lds + LDS_E2F + (row * E2_PITCH + lane * 4) * 4);
        float cp[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float4 w = wc[k];
            cp[k] = wave_sum(e.x * w.x + e.y * w.y + e.z * w.z + e.w * w.w) + bcv[k];
        }
        const float cc[4] = {cp[0] * cp[2], cp[1] * cp[2], cp[2], 1.0f};
        float pt[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = acc + __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(mi), 16 * i + a * 4 + k)) * cc[k];
            pt[a] = acc;
        }
        const float n0 = (pt[0] - p.pc0) / p.pd0, n1 = (pt[1] - p.pc1) / p.pd1, n2 = (pt[2] - p.pc2) / p.pd2;
        if (live && lane < 3) {
            p.center[r * 3 + lane] = cp[lane];
            p.xyz[r * 3 + lane] = pt[lane];
            p.ref[r * 3 + lane] = lane == 0 ? n0 : (lane == 1 ? n1 : n2);
        }
        const float two_pi = 6.283185307179586f;
        const float py = n1 * two_pi, px = n0 * two_pi, pz = n2 * two_pi;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int axis = j >> 1, ch = 128 * axis + 2 * lane + (j & 1);
            const float pos = axis == 0 ? py : (axis == 1 ? px : pz);
            const float a = pos / ((j & 1) ? dt.y : dt.x);
            const float v = (j & 1) ? cosf(a) : sinf(a);
            if (live) p.posemb[(long long)r * 384 + ch] = v;
            put_q16(lds + LDS_E1H, lds + LDS_E1L, 1024, row, ch, v);       // (the enc1 images: their readers passed the barrier above)
        }
    }
    __syncthreads();
    // ---- query_embedding.0 + ReLU -> hidden images (over the enc2 tile)
    load_bias2(bv, p.q0b);
    zero_acc<2>(a0, a1);
    phase<2, 12, B_Q0, 2>(a0, a1, rg, w_q0, 0, w_q2, 0, lane16, x1024());
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int fr = fresh(lane) & 15, fg = fresh(lane) >> 4;
        const int col = (2 * wave + j) * 16 + fr;
        const float b = bv[j];
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) put_q16(lds + LDS_HH, lds + LDS_HL, 512, 16 * t + 4 * fg + r, col, relu_f((a0[j][t][r] + a1[j][t][r]) + b));
    }
    __syncthreads();
    // ---- query_embedding.2
    load_bias2(bv, p.q2b);
    zero_acc<2>(a0, a1);
    phase<2, 8, B_Q2, 0>(a0, a1, rg, w_q2, 0, w_q2, 0, lane16, x512(LDS_HH, LDS_HL - LDS_HH));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int fr = fresh(lane) & 15, fg = fresh(lane) >> 4;
        const int col = (2 * wave + j) * 16 + fr;
        const float b = bv[j];
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + 16 * t + 4 * fg + r;
                if (m < p.R) p.qpos[(long long)m * C + col] = (a0[j][t][r] + a1[j][t][r]) + b;
            }
    }
}

}  // namespace

extern "C" int mv2d_qg_tail_x3(const float* x2, const float* enc, int ld_enc, const void* fc_hi, const void* fc_lo, const float* fc_b,
                               const void* e0_hi, const void* e0_lo, const float* e0_b, const void* e2_hi, const void* e2_lo,
                               const float* e2_b, const float* Wc, const float* bc, const float* minv, const float* dim_t,
                               const float* pc_range, const void* W0_hi, const void* W0_lo, const float* b0, const void* W2_hi,
                               const void* W2_lo, const float* b2, float* center, float* xyz, float* ref, float* posemb, float* qpos, int R,
                               void* stream) {
    MV2D_CHECK_ARG(x2 && enc && fc_hi && fc_lo && fc_b && e0_hi && e0_lo && e0_b && e2_hi && e2_lo && e2_b && Wc && bc && minv && dim_t &&
                       pc_range && W0_hi && W0_lo && b0 && W2_hi && W2_lo && b2 && center && xyz && ref && posemb && qpos,
                   "mv2d_qg_tail_x3: null pointer");
    MV2D_CHECK_ARG(ld_enc >= 1056 && ld_enc % 4 == 0, "mv2d_qg_tail_x3: ld_enc must be >= 1056 and a multiple of 4");
    MV2D_CHECK_ARG(R >= 0, "mv2d_qg_tail_x3: R < 0");
    if (R == 0) return MV2D_OK;
    typedef const uint4* U;
    QgTailParams p{x2, enc, ld_enc, (U)fc_hi, (U)fc_lo, fc_b, (U)e0_hi, (U)e0_lo, e0_b, (U)e2_hi, (U)e2_lo, e2_b, Wc, bc, minv, dim_t,
                   pc_range[0], pc_range[1], pc_range[2], pc_range[3] - pc_range[0], pc_range[4] - pc_range[1], pc_range[5] - pc_range[2],
                   (U)W0_hi, (U)W0_lo, b0, (U)W2_hi, (U)W2_lo, b2, center, xyz, ref, posemb, qpos, R, cdiv(R, 32)};
    // 64 L2-warming blocks (8 per XCD) behind the compute blocks of a launch that fills at least a quarter of the chip (measured at 150 blocks)
    const int helpers = p.nwork >= 64 ? 64 : 0;
    hipLaunchKernelGGL(qg_tail_x3_kernel, dim3(p.nwork + helpers), dim3(512), 0, (hipStream_t)stream, p);
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}
