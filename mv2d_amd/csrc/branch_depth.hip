// The prediction branches with a run-time number n of hidden layers (the reference head's num_reg_fcs, cross_attention_head.py:88,128-146):
//
//   class branch        n x [Linear(256,256) + LayerNorm + ReLU] + Linear(256,NC)
//   Sequential reg      n x [Linear(256,256) + ReLU]             + Linear(256,10)  + box-code tail
//   RegLayer reg        n x [Linear(256,256) + ReLU] shared, then per group g: Linear(256,256) + ReLU + Linear(256,d_g), + box-code tail
//
// heads_depth_x3_kernel has the block structure of heads_fused_x3_kernel (rowblock.hip), reg_layer_depth_x3_kernel that of reg_layer_x3_kernel
// (reglayer.hip); the hidden layers run as a loop over n with the weights stacked [L][n].  Per (row, layer) the arithmetic and its order are
// those of the two shipped kernels (at n = 2 the results are bit for bit theirs) and depend on neither M nor the row tiles per block.
// Every matrix is read as a uniform base plus one 32-bit lane offset (load_w_x3_uniform of reglayer.hip): per-lane 64-bit addresses next to
// the 64 fragment registers spill at RT = 4.
// LDS: 32 KB per row tile (+ 10 KB in the RegLayer kernel: 138 KB at RT = 4).
#include "x3_tile.h"

namespace {

__device__ __forceinline__ void load_wx3(BFrag wh[8], BFrag wl[8], const unsigned short* __restrict__ Wh, const unsigned short* __restrict__ Wl,
                                         unsigned lane_off) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {                 // fragment-major [k-step][16 column tiles][lane][8]
        wh[s].u = *reinterpret_cast<const uint4*>(Wh + s * (16 * 64 * 8) + lane_off);
        wl[s].u = *reinterpret_cast<const uint4*>(Wl + s * (16 * 64 * 8) + lane_off);
    }
}

// LayerNorm of one 256-wide row held 4 values per lane (the statement of rowblock.hip's ln_row)
__device__ __forceinline__ float4 ln_row4(float4 v, const float* __restrict__ w, const float* __restrict__ b, int c0, float eps) {
    const float mean = wave_sum(v.x + v.y + v.z + v.w) * (1.0f / C);
    const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
    const float var = wave_sum(dx * dx + dy * dy + dz * dz + dw * dw) * (1.0f / C);
    const float rstd = 1.0f / sqrtf(var + eps);
    const float4 ww = *reinterpret_cast<const float4*>(w + c0), bb = *reinterpret_cast<const float4*>(b + c0);
    return make_float4(dx * rstd * ww.x + bb.x, dy * rstd * ww.y + bb.y, dz * rstd * ww.z + bb.z, dw * rstd * ww.w + bb.w);
}

// cross_attention_head.py:219-238: add inverse_sigmoid(ref) to (cx, cy) and cz, sigmoid, de-normalise; T head: v / dt (mv2d_t_head.py:136-140)
struct BoxTail {
    const float* ref; float pc0, pc1, pc2, pd0, pd1, pd2, dt; const float* dt_rows;
};

__device__ __forceinline__ float box_code_col(const BoxTail& b, float v, int m, int o) {
    if (o == 0 || o == 1 || o == 4) {
        const int k = o == 4 ? 2 : o;
        const float x = fminf(fmaxf(b.ref[m * 3 + k], 0.f), 1.f);
        const float is = logf(fmaxf(x, 1e-5f) / fmaxf(1.f - x, 1e-5f));
        const float sg = 1.f / (1.f + expf(-(v + is)));
        v = o == 0 ? sg * b.pd0 + b.pc0 : (o == 1 ? sg * b.pd1 + b.pc1 : sg * b.pd2 + b.pc2);
    } else if (o >= 8) {
        const float dt = b.dt_rows ? b.dt_rows[m] : b.dt;
        if (dt != 0.f) v = v / dt;
    }
    return v;
}

struct HeadsDepthParams {
    const float* outs;
    // hidden layers, stacked [L][n]: fragment-major hi / lo matrices, biases [256]; LayerNorm weight / bias [256] (class branch only)
    const unsigned short* ch; const unsigned short* cl; const float* cb; const float* clnw; const float* clnb;
    const float* cwo; const float* cbo;                                           // class output layer [L][NC][256], [L][NC]
    const unsigned short* rh; const unsigned short* rl; const float* rb;
    const float* rwo; const float* rbo;                                           // regression output layer [L][10][256], [L][10]
    float* cls; float* reg;
    int M, L, n, NC; float eps;
    BoxTail tail;
};

// RT row tiles per block and CT class column tiles as in heads_fused_x3_kernel: wave w finishes row tile w % RT and class tile w / RT
template <int RT, int CT>
__global__ __launch_bounds__(1024) void heads_depth_x3_kernel(HeadsDepthParams p) {
    static_assert(RT * CT <= 16, "one wave per (row tile, class tile)");
    // one allocation with the hi / lo images first: every (tile, k-step) read of them is then one base register plus an immediate below 64 KB
    __shared__ __attribute__((aligned(16))) unsigned char smem[RT * 16 * 512 * 2 + RT * 16 * C * 4];
    unsigned char* const ah = smem;
    unsigned char* const al = smem + RT * 16 * 512;
    float* const tb = reinterpret_cast<float*>(smem + RT * 16 * 512 * 2);
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave-uniform by construction: row and bias addresses stay scalar
    // the row blocks of one (layer, branch) run on ONE XCD
    const int lin = xcd_chunked(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), gridDim.x * gridDim.y * gridDim.z);
    const int mb = (lin % gridDim.x) * (16 * RT), l = (lin / gridDim.x) % gridDim.y, branch = lin / (gridDim.x * gridDim.y);
    const long long h0 = (long long)l * p.n;                             // first hidden layer of decoder layer l in the [L][n] stacks
    const unsigned short* Wh = (branch == 0 ? p.ch : p.rh) + h0 * C * C;
    const unsigned short* Wl = (branch == 0 ? p.cl : p.rl) + h0 * C * C;
    const float* Bh = (branch == 0 ? p.cb : p.rb) + h0 * C;
    float4 av[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t)
        av[t] = *reinterpret_cast<const float4*>(p.outs + ((long long)l * p.M + min(mb + 16 * t + wave, p.M - 1)) * C + lane * 4);
    const unsigned woff = (unsigned)tid * 8u;                            // (16-column tile = wave, lane) in a k-step of a fragment-major matrix
    BFrag wh[8], wl[8];
    load_wx3(wh, wl, Wh, Wl, woff);
    const int aoff = wave * 512 + (((lane >> 1) ^ wave) << 4) + (lane & 1) * 8;     // this thread's 4 values in the 16-bit images of a tile
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        uint2 hi, lo;
        split4(av[t], hi, lo);
        *reinterpret_cast<uint2*>(ah + t * 8192 + aoff) = hi;
        *reinterpret_cast<uint2*>(al + t * 8192 + aoff) = lo;
    }
    __syncthreads();
    const int col = wave * 16 + fr;
    float* trow = tb + wave * C + ((lane ^ (wave & 15)) << 2);          // row = wave of a tile, columns 4 lane ..
    // ---- n x [linear -> (LayerNorm) -> ReLU]: every layer but the last back into the hi / lo images, the last kept as the fp32 tile
#pragma unroll 1
    for (int i = 0; i < p.n; ++i) {
        const bool last = i + 1 == p.n;
        f32x4_t acc[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t] = tile_mma_x3(ah + t * 8192, al + t * 8192, wh, wl, fr, fg);
        __builtin_amdgcn_sched_barrier(0);              // the fragments are dead here: the next matrix reuses their registers
        // in flight during the row stage.  Unconditional (behind the last layer: the same matrix again, never used): a conditional load makes
        // the 64 fragment registers live in both their old and their new value across the loop's back edge, and the kernel spills
        const int nx = min(i + 1, p.n - 1);
        load_wx3(wh, wl, Wh + (long long)nx * C * C, Wl + (long long)nx * C * C, woff);
        {
            const float b = Bh[i * C + col];
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) tb[t * 16 * C + toff(4 * fg + r, col)] = acc[t][r] + b;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            float4 v = *reinterpret_cast<float4*>(trow + t * 16 * C);
            if (branch == 0) v = ln_row4(v, p.clnw + (h0 + i) * C, p.clnb + (h0 + i) * C, lane * 4, p.eps);
            v = make_float4(relu_f(v.x), relu_f(v.y), relu_f(v.z), relu_f(v.w));
            if (last) {
                *reinterpret_cast<float4*>(trow + t * 16 * C) = v;
            } else {
                uint2 hi, lo;
                split4(v, hi, lo);
                *reinterpret_cast<uint2*>(ah + t * 8192 + aoff) = hi;
                *reinterpret_cast<uint2*>(al + t * 8192 + aoff) = lo;
            }
        }
        __syncthreads();
    }
    // the reg branch has one column tile (10 wide), the cls branch CT
    if (wave >= (branch == 0 ? CT * RT : RT)) return;
    const int rt = CT == 1 ? wave : wave % RT, ct = CT == 1 ? 0 : wave / RT;
    const int m0 = mb + 16 * rt;
    if (m0 >= p.M) return;
    const float* tbt = tb + rt * 16 * C;
    // ---- final Linear(256 -> NC | 10), exact fp32: 16x16 tile ct, weight rows >= nout clamped and masked
    const int nout = branch == 0 ? p.NC : 10;
    const float* wlast = branch == 0 ? p.cwo + (long long)l * nout * C : p.rwo + (long long)l * 10 * C;
    const float* blast = branch == 0 ? p.cbo + l * nout : p.rbo + l * 10;
    float* outp = branch == 0 ? p.cls : p.reg;
    const int n = 16 * ct + fr;                                         // this lane's output column
    __builtin_amdgcn_sched_barrier(0);
    Frag f;
    load_w(f, wlast, C, n, nout, fg);
    const f32x4_t o = tile_mma(tbt, f, fr, fg);
    if (n >= nout) return;
    const float b = blast[n];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + 4 * fg + r;
        if (m >= p.M) continue;
        float v = o[r] + b;
        if (branch == 1) v = box_code_col(p.tail, v, m, fr);
        outp[((long long)l * p.M + m) * nout + n] = v;
    }
}

struct RegLayerDepthParams {
    const float* outs;
    const unsigned short* sh; const unsigned short* sl; const float* sb;         // shared layers, stacked [L][n]
    const unsigned short* t1h; const unsigned short* t1l; const float* tb1;      // task heads, first layers: [L][G]
    const float* t2; const float* tb2;                                           // second layers: [L][10][256] (row o: the group of column o), [L][10]
    float* reg;
    int M, L, n, G;
    unsigned long long gstart;            // 4 bits per group boundary: columns of group g = [nib(g), nib(g + 1)), nib(G) = 10
    BoxTail tail;
};

template <int RT>
__global__ __launch_bounds__(1024) void reg_layer_depth_x3_kernel(RegLayerDepthParams p) {
    // (one allocation, the images first: see heads_depth_x3_kernel; with three separate arrays the RT = 4 instance keeps ~60 precomputed LDS
    // addresses and spills them)
    __shared__ __attribute__((aligned(16))) unsigned char smem[RT * 16 * 512 * 2 + RT * 16 * C * 4 + 10 * C * 4];
    unsigned char* const ah = smem;
    unsigned char* const al = smem + RT * 16 * 512;
    // (the tile's offset goes through a register the compiler cannot see into: it then keeps ONE address per accumulator row plus the tile's
    // immediate, not one folded address per (row, tile))
    unsigned tb_off = RT * 16 * 512 * 2;
    asm volatile("" : "+s"(tb_off));
    float* const tb = reinterpret_cast<float*>(smem + tb_off);
    float* const w2s = tb + RT * 16 * C;
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave-uniform by construction: row and bias addresses stay scalar
    const int lin = xcd_chunked(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
    const int mb = (lin % gridDim.x) * (16 * RT), l = lin / gridDim.x;
    const long long h0 = (long long)l * p.n, g0 = (long long)l * p.G;
    const unsigned short* Sh = p.sh + h0 * C * C;
    const unsigned short* Sl = p.sl + h0 * C * C;
    const unsigned short* Th = p.t1h + g0 * C * C;
    const unsigned short* Tl = p.t1l + g0 * C * C;
    float4 av[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t)
        av[t] = *reinterpret_cast<const float4*>(p.outs + ((long long)l * p.M + min(mb + 16 * t + wave, p.M - 1)) * C + lane * 4);
    const unsigned woff = (unsigned)tid * 8u;
    BFrag wh[8], wl[8];
    load_wx3(wh, wl, Sh, Sl, woff);
    if (tid < 10 * C / 4) *reinterpret_cast<float4*>(w2s + 4 * tid) = *reinterpret_cast<const float4*>(p.t2 + (long long)l * 10 * C + 4 * tid);
    const int aoff = wave * 512 + (((lane >> 1) ^ wave) << 4) + (lane & 1) * 8;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        uint2 hi, lo;
        split4(av[t], hi, lo);
        *reinterpret_cast<uint2*>(ah + t * 8192 + aoff) = hi;
        *reinterpret_cast<uint2*>(al + t * 8192 + aoff) = lo;
    }
    __syncthreads();
    const int col = wave * 16 + fr;
    float* trow = tb + wave * C + ((lane ^ (wave & 15)) << 2);
    f32x4_t acc[RT];
    // ---- the n shared layers: linear -> ReLU -> hi / lo images
#pragma unroll 1
    for (int s = 0; s < p.n; ++s) {
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t] = tile_mma_x3(ah + t * 8192, al + t * 8192, wh, wl, fr, fg);
        __builtin_amdgcn_sched_barrier(0);
        // in flight during the row stage: the next shared layer, behind the last one the first task head
        if (s + 1 < p.n) load_wx3(wh, wl, Sh + (long long)(s + 1) * C * C, Sl + (long long)(s + 1) * C * C, woff);
        else load_wx3(wh, wl, Th, Tl, woff);
        {
            const float b = p.sb[(h0 + s) * C + col];
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) tb[t * 16 * C + toff(4 * fg + r, col)] = acc[t][r] + b;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            float4 v = *reinterpret_cast<float4*>(trow + t * 16 * C);
            v = make_float4(relu_f(v.x), relu_f(v.y), relu_f(v.z), relu_f(v.w));
            uint2 hi, lo;
            split4(v, hi, lo);
            *reinterpret_cast<uint2*>(ah + t * 8192 + aoff) = hi;
            *reinterpret_cast<uint2*>(al + t * 8192 + aoff) = lo;
        }
        __syncthreads();
    }
    // ---- the task heads: h_g = ReLU(T1_g reg_feat) through the fp32 tile, then the group's output columns; lane o keeps column o of its row
    float outv[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) outv[t] = 0.f;
#pragma unroll 1
    for (int g = 0; g < p.G; ++g) {
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t] = tile_mma_x3(ah + t * 8192, al + t * 8192, wh, wl, fr, fg);
        __builtin_amdgcn_sched_barrier(0);
        const int gx = min(g + 1, p.G - 1);                             // (unconditional, see heads_depth_x3_kernel)
        load_wx3(wh, wl, Th + (long long)gx * C * C, Tl + (long long)gx * C * C, woff);
        const float b = p.tb1[(g0 + g) * C + col];
        if (g > 0) __syncthreads();                                     // the row stage of group g - 1 has read the tile
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) tb[t * 16 * C + toff(4 * fg + r, col)] = acc[t][r] + b;
        __syncthreads();
        const int o0 = (int)((p.gstart >> (4 * g)) & 15), o1 = (int)((p.gstart >> (4 * g + 4)) & 15);
        // (the row is read from the tile again for every output column: holding the RT rows of a lane next to the 64 fragment registers in
        // flight is what makes reg_layer_x3_kernel<4> spill)
#pragma unroll 1
        for (int o = o0; o < o1; ++o) {
            const float4 w = *reinterpret_cast<const float4*>(w2s + o * C + 4 * lane);
#pragma unroll
            for (int t = 0; t < RT; ++t) {                              // RT independent reductions side by side
                const float4 x = *reinterpret_cast<float4*>(trow + t * 16 * C);
                const float4 v = make_float4(relu_f(x.x), relu_f(x.y), relu_f(x.z), relu_f(x.w));
                const float s = wave_sum((v.x * w.x + v.y * w.y) + (v.z * w.z + v.w * w.w));
                if (lane == o) outv[t] = s;
            }
        }
    }
    if (lane >= 10) return;
    const float b2 = p.tb2[l * 10 + lane];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const int m = mb + 16 * t + wave;
        if (m >= p.M) continue;
        p.reg[((long long)l * p.M + m) * 10 + lane] = box_code_col(p.tail, outv[t] + b2, m, lane);
    }
}

// branches = 2: the class and the regression branch (gridDim.z = 2); branches = 1: the class branch alone (branch is 0 in every block: the
// regression tables, ref, reg and the tail are never touched)
int heads_depth_launch(const float* outs, const void* const* cls_w, const void* const* reg_w, const float* ref, float* cls,
                       float* reg, int M, int L, int n_fcs, int num_classes, float eps, const float* pc_range, float dt, const float* dt_rows,
                       void* stream, int branches) {
    const bool two = branches == 2, cls_only = !two;                    // (every message carries the name of the entry that was called)
    MV2D_CHECK_ARG(outs && cls_w && cls && L > 0 && M >= 0 && (cls_only || (reg_w && ref && reg && pc_range)),
                   cls_only ? "mv2d_heads_cls_depth_x3: null pointer or bad size" : "mv2d_heads_depth_x3: null pointer or bad size");
    MV2D_CHECK_ARG(n_fcs >= 1 && n_fcs <= 3,
                   cls_only ? "mv2d_heads_cls_depth_x3: n_fcs (num_reg_fcs) must be in [1, 3]" : "mv2d_heads_depth_x3: n_fcs (num_reg_fcs) must be in [1, 3]");
    MV2D_CHECK_ARG(num_classes >= 1 && num_classes <= 64,
                   cls_only ? "mv2d_heads_cls_depth_x3: num_classes must be in [1, 64]" : "mv2d_heads_depth_x3: num_classes must be in [1, 64]");
    for (int i = 0; i < 7; ++i)
        MV2D_CHECK_ARG(cls_w[i] != nullptr, cls_only ? "mv2d_heads_cls_depth_x3: null cls weight" : "mv2d_heads_depth_x3: null cls weight");
    for (int i = 0; i < 5 && two; ++i) MV2D_CHECK_ARG(reg_w[i] != nullptr, "mv2d_heads_depth_x3: null reg weight");
    if (M == 0) return MV2D_OK;
    typedef const unsigned short* U; typedef const float* Fp;
    HeadsDepthParams p{};
    p.outs = outs;
    p.ch = (U)cls_w[0]; p.cl = (U)cls_w[1]; p.cb = (Fp)cls_w[2]; p.clnw = (Fp)cls_w[3]; p.clnb = (Fp)cls_w[4]; p.cwo = (Fp)cls_w[5]; p.cbo = (Fp)cls_w[6];
    if (two) {
        p.rh = (U)reg_w[0]; p.rl = (U)reg_w[1]; p.rb = (Fp)reg_w[2]; p.rwo = (Fp)reg_w[3]; p.rbo = (Fp)reg_w[4];
        p.reg = reg;
        p.tail = BoxTail{ref, pc_range[0], pc_range[1], pc_range[2], pc_range[3] - pc_range[0], pc_range[4] - pc_range[1], pc_range[5] - pc_range[2],
                         dt, dt_rows};
    }
    p.cls = cls;
    p.M = M; p.L = L; p.n = n_fcs; p.NC = num_classes; p.eps = eps;
    const int ct = (num_classes + 15) / 16;                             // class column tiles
    const hipStream_t st = (hipStream_t)stream;
#define MV2D_HEADS_DEPTH(RT)                                                                                                            \
    switch (ct) {                                                                                                                     \
        case 1: hipLaunchKernelGGL((heads_depth_x3_kernel<RT, 1>), dim3(cdiv(M, 16 * RT), L, branches), dim3(1024), 0, st, p); break;       \
        case 2: hipLaunchKernelGGL((heads_depth_x3_kernel<RT, 2>), dim3(cdiv(M, 16 * RT), L, branches), dim3(1024), 0, st, p); break;       \
        case 3: hipLaunchKernelGGL((heads_depth_x3_kernel<RT, 3>), dim3(cdiv(M, 16 * RT), L, branches), dim3(1024), 0, st, p); break;       \
        default: hipLaunchKernelGGL((heads_depth_x3_kernel<RT, 4>), dim3(cdiv(M, 16 * RT), L, branches), dim3(1024), 0, st, p); break;      \
    }
    // the row-tile rule of mv2d_heads_fused_x3_nc
    if (M <= 512) { MV2D_HEADS_DEPTH(1) }
    else if (M <= 1024) { MV2D_HEADS_DEPTH(2) }
    else { MV2D_HEADS_DEPTH(4) }
#undef MV2D_HEADS_DEPTH
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}

}  // namespace

extern "C" int mv2d_heads_depth_x3(const float* outs, const void* const* cls_w, const void* const* reg_w, const float* ref, float* cls, float* reg,
                                   int M, int L, int n_fcs, int num_classes, float eps, const float* pc_range, float dt, const float* dt_rows,
                                   void* stream) {
    // cls_w: {w_hi, w_lo, b, ln_w, ln_b, w_out, b_out}; reg_w: {w_hi, w_lo, b, w_out, b_out} device pointers (include/mv2d_hip.h)
    return heads_depth_launch(outs, cls_w, reg_w, ref, cls, reg, M, L, n_fcs, num_classes, eps, pc_range, dt, dt_rows, stream, 2);
}

extern "C" int mv2d_heads_cls_depth_x3(const float* outs, const void* const* cls_w, float* cls, int M, int L, int n_fcs, int num_classes, float eps,
                                       void* stream) {
    return heads_depth_launch(outs, cls_w, nullptr, nullptr, cls, nullptr, M, L, n_fcs, num_classes, eps, nullptr, 0.f,
                              nullptr, stream, 1);
}

extern "C" int mv2d_reg_layer_depth_x3(const float* outs, const void* const* w, const float* ref, float* reg, int M, int L, int n_fcs, int n_groups,
                                       const int* group_dims, const float* pc_range, float dt, const float* dt_rows, void* stream) {
    // w: {s_hi, s_lo, s_b, t1_hi, t1_lo, t1_b, t2_w, t2_b} device pointers (include/mv2d_hip.h); group_dims is read here, on the host
    MV2D_CHECK_ARG(outs && w && ref && reg && group_dims && pc_range && L > 0 && M >= 0, "mv2d_reg_layer_depth_x3: null pointer or bad size");
    MV2D_CHECK_ARG(n_fcs >= 1 && n_fcs <= 3, "mv2d_reg_layer_depth_x3: n_fcs (num_reg_fcs) must be in [1, 3]");
    MV2D_CHECK_ARG(n_groups >= 1 && n_groups <= 10, "mv2d_reg_layer_depth_x3: n_groups must be in [1, 10]");
    unsigned long long gstart = 0;
    int sum = 0;
    for (int g = 0; g < n_groups; ++g) {
        MV2D_CHECK_ARG(group_dims[g] >= 1 && group_dims[g] <= 10, "mv2d_reg_layer_depth_x3: every group_dims entry must be at least 1 (and the sum 10)");
        gstart |= (unsigned long long)sum << (4 * g);
        sum += group_dims[g];
        MV2D_CHECK_ARG(sum <= 10, "mv2d_reg_layer_depth_x3: group_dims must sum to 10, the box code size");
    }
    MV2D_CHECK_ARG(sum == 10, "mv2d_reg_layer_depth_x3: group_dims must sum to 10, the box code size");
    gstart |= 10ull << (4 * n_groups);
    for (int i = 0; i < 8; ++i) MV2D_CHECK_ARG(w[i] != nullptr, "mv2d_reg_layer_depth_x3: null weight");
    if (M == 0) return MV2D_OK;
    typedef const unsigned short* U; typedef const float* Fp;
    RegLayerDepthParams p{outs, (U)w[0], (U)w[1], (Fp)w[2], (U)w[3], (U)w[4], (Fp)w[5], (Fp)w[6], (Fp)w[7], reg, M, L, n_fcs, n_groups, gstart,
                          BoxTail{ref, pc_range[0], pc_range[1], pc_range[2], pc_range[3] - pc_range[0], pc_range[4] - pc_range[1],
                                  pc_range[5] - pc_range[2], dt, dt_rows}};
    const hipStream_t st = (hipStream_t)stream;
    if (M <= 512) hipLaunchKernelGGL((reg_layer_depth_x3_kernel<1>), dim3(cdiv(M, 16), L), dim3(1024), 0, st, p);
    else if (M <= 1024) hipLaunchKernelGGL((reg_layer_depth_x3_kernel<2>), dim3(cdiv(M, 32), L), dim3(1024), 0, st, p);
    else hipLaunchKernelGGL((reg_layer_depth_x3_kernel<4>), dim3(cdiv(M, 64), L), dim3(1024), 0, st, p);
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}
