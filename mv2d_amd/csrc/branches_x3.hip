// The box head's prediction branches in split precision, with n hidden layers (the reference head's num_reg_fcs, cross_attention_head.py:88,
// 128-146; the RegLayer: :52-83, use_reg_layer):
//
//   class branch        n x [Linear(256,256) + LayerNorm + ReLU] + Linear(256,NC)
//   Sequential reg      n x [Linear(256,256) + ReLU]             + Linear(256,10)  + box-code tail
//   RegLayer reg        n x [Linear(256,256) + ReLU] shared, then per group g: Linear(256,256) + ReLU + Linear(256,d_g), + box-code tail
//
// heads_x3_kernel runs the first two, reg_layer_x3_kernel the third.  One block of 16 waves owns RT row tiles (16 rows each) of one (decoder
// layer, branch): wave w computes column tile w of a 256x256 linear (bf16x3 on v_mfma_f32_16x16x32, ~1e-5 relative; the fragments of the NEXT
// matrix in flight behind the row stage of the current one) and owns row w of every tile in the LayerNorm / ReLU stages.  The RT tiles share
// one load of the weight fragments: with many rows (a batch of samples) the kernels are bound by the L2 -> CU traffic of the weights (0.5 MB
// per block), not by the matrix pipe.  The output layers stay exact fp32.  Per (row, layer) the arithmetic and its order depend on neither M,
// nor RT, nor on how the depth reaches the kernel.
//
// The depth reaches it as NF: NF = 2 is the depth every shipped config has, as a compile-time constant (the hidden-layer loop unrolls, each
// layer through its own pointers, nothing loaded behind the last one); NF = 0 is a run-time loop over p.n.  Two table layouts feed both: the
// first entries' (mv2d_heads_fused_x3*, mv2d_heads_cls_x3_nc, mv2d_reg_layer_x3: one [L] array per hidden layer) and the *_depth_x3
// entries' (one [L][n] array for all of them); at depth 2 either layout runs the NF = 2 instances.
// Every matrix is read as a uniform base plus one 32-bit lane offset (load_w_x3_uniform), and LDS is one allocation with the hi / lo images
// first: per-lane 64-bit addresses or one folded LDS address per (row, tile) next to the 64 fragment registers spill at RT = 4
// (profiles/branches_x3_kernel_stats.txt).
// LDS: 32 KB per row tile (+ 10 KB in the RegLayer kernel: 138 KB at RT = 4).
#include <cstdio>

#include "x3_tile.h"

namespace {

// One hidden Linear(256,256) for all decoder layers: fragment-major hi / lo matrices, biases [256].  Decoder layer l's lies l * stride
// matrices (biases) behind the pointers: stride 1 in an [L] array, n in an [L][n] one
struct X3Layers { const unsigned short* h; const unsigned short* l; const float* b; };

// hidden layer i of a stack: with the depth a constant, layers 0 and 1 by their own pointers (i is a constant once the loop is unrolled);
// in the run-time loop i steps behind layer 0 in the [L][n] array.  (Never a kernel-argument array indexed by a run-time i: that copies the
// arguments to scratch.)
template <int NF, typename T>
__device__ __forceinline__ const T* hidden(const T* p0, const T* p1, int i, int step) {
    return NF ? (i == 0 ? p0 : p1) : p0 + (long long)i * step;
}

struct HeadsX3Params {
    const float* outs;
    X3Layers c0, c1;                                                              // class branch, hidden layers 0 and 1
    const float* ln0w; const float* ln0b; const float* ln1w; const float* ln1b;   // their LayerNorm weight / bias [256], strided alike
    const float* cwo; const float* cbo;                                           // class output layer [L][NC][256], [L][NC]
    X3Layers r0, r1;                                                              // regression branch
    const float* rwo; const float* rbo;                                           // regression output layer [L][10][256], [L][10]
    float* cls; float* reg;
    int M, L, n, stride, NC; float eps;
    BoxTail tail;
};

// CT = 16-column tiles of the class output layer (NC <= 16 CT): wave w finishes row tile w % RT and class tile w / RT, so the waves that sit
// idle behind the last 256x256 linear at CT = 1 carry the extra class tiles (RT * CT <= 16: up to 64 classes at RT = 4).
// NCF = the class count as a compile-time constant (the 10-class launch), 0 = p.NC.  NF = the depth likewise, 0 = p.n.
template <int RT, int CT, int NCF, int NF>
__global__ __launch_bounds__(1024) void heads_x3_kernel(HeadsX3Params p) {
    static_assert(RT * CT <= 16, "one wave per (row tile, class tile)");
    // one allocation with the hi / lo images first: every (tile, k-step) read of them is then one base register plus an immediate below 64 KB
    __shared__ __attribute__((aligned(16))) unsigned char smem[RT * 16 * 512 * 2 + RT * 16 * C * 4];
    unsigned char* const ah = smem;
    unsigned char* const al = smem + RT * 16 * 512;
    float* const tb = reinterpret_cast<float*>(smem + RT * 16 * 512 * 2);
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave-uniform by construction: row and bias addresses stay scalar
    // the row blocks of one (layer, branch) run on ONE XCD: its 1 MB of weights is fetched by ~2 XCDs instead of all 8
    const int lin = xcd_chunked(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), gridDim.x * gridDim.y * gridDim.z);
    const int mb = (lin % gridDim.x) * (16 * RT), l = (lin / gridDim.x) % gridDim.y, branch = lin / (gridDim.x * gridDim.y);
    const int n = NF ? NF : p.n;
    constexpr int UNROLL = NF ? NF : 1;                                  // of the hidden layers' loop: all of it, or none
    const long long h0 = (long long)l * p.stride;                        // decoder layer l in the hidden layers' arrays
    const unsigned short* W0h = (branch == 0 ? p.c0.h : p.r0.h) + h0 * C * C;
    const unsigned short* W0l = (branch == 0 ? p.c0.l : p.r0.l) + h0 * C * C;
    const unsigned short* W1h = (branch == 0 ? p.c1.h : p.r1.h) + h0 * C * C;
    const unsigned short* W1l = (branch == 0 ? p.c1.l : p.r1.l) + h0 * C * C;
    const float* B0 = (branch == 0 ? p.c0.b : p.r0.b) + h0 * C;
    const float* B1 = (branch == 0 ? p.c1.b : p.r1.b) + h0 * C;
    float4 av[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t)
        av[t] = *reinterpret_cast<const float4*>(p.outs + ((long long)l * p.M + min(mb + 16 * t + wave, p.M - 1)) * C + lane * 4);
    const unsigned woff = (unsigned)tid * 8u;                            // (16-column tile = wave, lane) in a k-step of a fragment-major matrix
    BFrag wh[8], wl[8];
    load_w_x3_uniform(wh, wl, W0h, W0l, woff);
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
#pragma unroll UNROLL
    for (int i = 0; i < n; ++i) {
        const bool last = i + 1 == n;
        f32x4_t acc[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t] = tile_mma_x3(ah + t * 8192, al + t * 8192, wh, wl, fr, fg);
        // The fragments are dead here: the next matrix reuses their registers, in flight during the row stage.  Where registers are short
        // (the run-time loop with its back edge, four row tiles) nothing may move across this point.  The unrolled kernels with one or two
        // row tiles have registers to spare; fenced, their launch of 6 layers x 900 rows takes 0.5 us of 25 longer
        if constexpr (NF == 0 || RT == 4) __builtin_amdgcn_sched_barrier(0);
        // The load is unconditional, behind the last layer the same matrix again, never used: under a run-time condition the 64 fragment
        // registers are live in both their old and their new value across the loop's back edge, and the NF = 0 kernels spill.  Unrolled
        // (NF = 2) the unused load is dropped as dead code.  (Written as `if (!last)` the same work comes out with another register
        // assignment, which spills 40 to 48 B/lane at RT = 4; this form spills nothing.)
        const int nx = min(i + 1, n - 1);
        load_w_x3_uniform(wh, wl, hidden<NF>(W0h, W1h, nx, C * C), hidden<NF>(W0l, W1l, nx, C * C), woff);
        {
            const float b = hidden<NF>(B0, B1, i, C)[col];
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) tb[t * 16 * C + toff(4 * fg + r, col)] = acc[t][r] + b;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            float4 v = *reinterpret_cast<float4*>(trow + t * 16 * C);
            if (branch == 0) v = ln_row(v, hidden<NF>(p.ln0w, p.ln1w, i, C) + h0 * C, hidden<NF>(p.ln0b, p.ln1b, i, C) + h0 * C, lane * 4, p.eps);
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
    const int nout = branch == 0 ? (NCF ? NCF : p.NC) : 10;
    const float* wlast = branch == 0 ? p.cwo + (long long)l * nout * C : p.rwo + (long long)l * 10 * C;
    const float* blast = branch == 0 ? p.cbo + l * nout : p.rbo + l * 10;
    float* outp = branch == 0 ? p.cls : p.reg;
    const int no = 16 * ct + fr;                                        // this lane's output column
    __builtin_amdgcn_sched_barrier(0);
    Frag f;
    load_w(f, wlast, C, no, nout, fg);
    const f32x4_t o = tile_mma(tbt, f, fr, fg);
    if (no >= nout) return;
    const float b = blast[no];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + 4 * fg + r;
        if (m >= p.M) continue;
        float v = o[r] + b;
        if (branch == 1) v = box_code_col(p.tail, v, m, fr);
        outp[((long long)l * p.M + m) * nout + no] = v;
    }
}

struct RegLayerX3Params {
    const float* outs;
    X3Layers s0, s1;                                                             // shared hidden layers 0 and 1
    X3Layers t1;                                                                 // task heads, first layers: [L][G]
    const float* t2; const float* tb2;                                           // second layers: [L][10][256] (row o: the group of column o), [L][10]
    float* reg;
    int M, L, n, stride, G;
    unsigned long long gstart;            // 4 bits per group boundary: columns of group g = [nib(g), nib(g + 1)), nib(G) = 10
    BoxTail tail;
};

// reg_feat (the output of the n shared layers) stays in the hi / lo LDS images for all G task heads; h_g = ReLU(T1_g reg_feat) goes through
// the fp32 tile, and the group's d_g output columns are exact fp32 dot products of the row with the rows of T2 (staged in LDS once:
// [10][256]), reduced over the wave -- so the output layer costs d_g wave reductions per row instead of one 64-MFMA chain per group on a
// single wave.
template <int RT, int NF>
__global__ __launch_bounds__(1024) void reg_layer_x3_kernel(RegLayerX3Params p) {
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
    // the row blocks of one layer run on ONE XCD (see heads_x3_kernel)
    const int lin = xcd_chunked(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
    const int mb = (lin % gridDim.x) * (16 * RT), l = lin / gridDim.x;
    const int n = NF ? NF : p.n;
    constexpr int UNROLL = NF ? NF : 1;                                  // of the hidden layers' loop: all of it, or none
    const long long h0 = (long long)l * p.stride, g0 = (long long)l * p.G;
    const unsigned short* S0h = p.s0.h + h0 * C * C;
    const unsigned short* S0l = p.s0.l + h0 * C * C;
    const unsigned short* S1h = p.s1.h + h0 * C * C;
    const unsigned short* S1l = p.s1.l + h0 * C * C;
    const unsigned short* Th = p.t1.h + g0 * C * C;
    const unsigned short* Tl = p.t1.l + g0 * C * C;
    float4 av[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t)
        av[t] = *reinterpret_cast<const float4*>(p.outs + ((long long)l * p.M + min(mb + 16 * t + wave, p.M - 1)) * C + lane * 4);
    const unsigned woff = (unsigned)tid * 8u;
    BFrag wh[8], wl[8];
    load_w_x3_uniform(wh, wl, S0h, S0l, woff);
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
#pragma unroll UNROLL
    for (int s = 0; s < n; ++s) {
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t] = tile_mma_x3(ah + t * 8192, al + t * 8192, wh, wl, fr, fg);
        __builtin_amdgcn_sched_barrier(0);
        // in flight during the row stage: the next shared layer, behind the last one the first task head
        if (s + 1 < n) load_w_x3_uniform(wh, wl, hidden<NF>(S0h, S1h, s + 1, C * C), hidden<NF>(S0l, S1l, s + 1, C * C), woff);
        else load_w_x3_uniform(wh, wl, Th, Tl, woff);
        {
            const float b = (hidden<NF>(p.s0.b, p.s1.b, s, C) + h0 * C)[col];
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
        const int gx = min(g + 1, p.G - 1);                             // (unconditional, see heads_x3_kernel)
        load_w_x3_uniform(wh, wl, Th + (long long)gx * C * C, Tl + (long long)gx * C * C, woff);
        const float b = p.t1.b[(g0 + g) * C + col];
        if (g > 0) __syncthreads();                                     // the row stage of group g - 1 has read the tile
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) tb[t * 16 * C + toff(4 * fg + r, col)] = acc[t][r] + b;
        __syncthreads();
        const int o0 = (int)((p.gstart >> (4 * g)) & 15), o1 = (int)((p.gstart >> (4 * g + 4)) & 15);
        // (the row is read from the tile again for every output column: holding the RT rows of a lane next to the 64 fragment registers in
        // flight spills at RT = 4)
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

typedef const unsigned short* U;
typedef const float* Fp;

// every message begins with the name of a C entry
int arg_error(const char* entry, const char* what) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s", entry, what);
    mv2d_set_error(msg);
    return MV2D_ERR_ARG;
}
#define X3_CHECK(cond, entry, what)                       \
    do {                                                  \
        if (!(cond)) return arg_error(entry, what);       \
    } while (0)

// hidden layers 0 and 1 of an [L][n] array (layer 1 unused at n = 1)
void stacked(X3Layers& l0, X3Layers& l1, const void* h, const void* l, const void* b) {
    l0 = X3Layers{(U)h, (U)l, (Fp)b};
    l1 = X3Layers{(U)h + C * C, (U)l + C * C, (Fp)b + C};
}

// The two table layouts (include/mv2d_hip.h).  PER_LAYER: the first entries', one [L] array per hidden layer, depth 2
//   cls_w {w0_hi,w0_lo,b0,lnw1,lnb1,w3_hi,w3_lo,b3,lnw4,lnb4,w6,b6}, reg_w {w0_hi,w0_lo,b0,w2_hi,w2_lo,b2,w4,b4}
//   RegLayer w {s1_hi,s1_lo,s1_b, s2_hi,s2_lo,s2_b, t1_hi,t1_lo,t1_b, t2_w,t2_b}
// STACKED: the depth entries', the hidden layers of a branch in one [L][n] array
//   cls_w {w_hi, w_lo, b, ln_w, ln_b, w_out, b_out}, reg_w {w_hi, w_lo, b, w_out, b_out}
//   RegLayer w {s_hi, s_lo, s_b, t1_hi, t1_lo, t1_b, t2_w, t2_b}
enum Tables { PER_LAYER, STACKED };

// The class and the Sequential regression branch from either layout (n_fcs is read with STACKED only).
// branches = 2: the class and the regression branch (gridDim.z = 2); branches = 1: the class branch alone (branch is 0 in every block: the
// regression tables, ref, reg and the tail are never touched and may be NULL).
// name: the entry that was called; name0: the name under which the first entries report a null argument (mv2d_heads_cls_x3_nc reports
// everything else as mv2d_heads_fused_x3, as it always has)
int heads_x3_launch(Tables tables, const char* name, const char* name0, const float* outs, const void* const* cls_w, const void* const* reg_w, const float* ref,
                    float* cls, float* reg, int M, int L, int n_fcs, int num_classes, float eps, const float* pc_range, float dt,
                    const float* dt_rows, void* stream, int branches) {
    const bool two = branches == 2, depth = tables == STACKED;
    const bool ptrs = outs && cls_w && cls && L > 0 && (!two || (reg_w && ref && reg && pc_range));
    if (depth) {
        X3_CHECK(ptrs && M >= 0, name, "null pointer or bad size");
        X3_CHECK(n_fcs >= 1 && n_fcs <= 3, name, "n_fcs (num_reg_fcs) must be in [1, 3]");
    } else {
        X3_CHECK(ptrs, name0, "null pointer");
    }
    X3_CHECK(num_classes >= 1 && num_classes <= 64, name, "num_classes must be in [1, 64]");
    for (int i = 0; i < (depth ? 7 : 12); ++i) X3_CHECK(cls_w[i] != nullptr, name, "null cls weight");
    for (int i = 0; i < (depth ? 5 : 8) && two; ++i) X3_CHECK(reg_w[i] != nullptr, name, "null reg weight");
    if (M == 0) return MV2D_OK;
    HeadsX3Params p{};
    p.outs = outs; p.cls = cls;
    p.M = M; p.L = L; p.NC = num_classes; p.eps = eps;
    if (depth) {
        p.n = p.stride = n_fcs;
        stacked(p.c0, p.c1, cls_w[0], cls_w[1], cls_w[2]);
        p.ln0w = (Fp)cls_w[3]; p.ln0b = (Fp)cls_w[4]; p.ln1w = p.ln0w + C; p.ln1b = p.ln0b + C;
        p.cwo = (Fp)cls_w[5]; p.cbo = (Fp)cls_w[6];
        if (two) {
            stacked(p.r0, p.r1, reg_w[0], reg_w[1], reg_w[2]);
            p.rwo = (Fp)reg_w[3]; p.rbo = (Fp)reg_w[4];
        }
    } else {
        p.n = 2; p.stride = 1;
        p.c0 = X3Layers{(U)cls_w[0], (U)cls_w[1], (Fp)cls_w[2]}; p.ln0w = (Fp)cls_w[3]; p.ln0b = (Fp)cls_w[4];
        p.c1 = X3Layers{(U)cls_w[5], (U)cls_w[6], (Fp)cls_w[7]}; p.ln1w = (Fp)cls_w[8]; p.ln1b = (Fp)cls_w[9];
        p.cwo = (Fp)cls_w[10]; p.cbo = (Fp)cls_w[11];
        if (two) {
            p.r0 = X3Layers{(U)reg_w[0], (U)reg_w[1], (Fp)reg_w[2]};
            p.r1 = X3Layers{(U)reg_w[3], (U)reg_w[4], (Fp)reg_w[5]};
            p.rwo = (Fp)reg_w[6]; p.rbo = (Fp)reg_w[7];
        }
    }
    if (two) {
        p.reg = reg;
        p.tail = box_tail(ref, pc_range, dt, dt_rows);
    }
    const bool nf2 = p.n == 2;
    const int ct = nf2 && num_classes == 10 ? 0 : (num_classes + 15) / 16;         // class column tiles (0: the 10-class instance, NF = 2 only)
    const hipStream_t st = (hipStream_t)stream;
#define X3_HEADS(RT, CT, NCF)                                                                                                    \
    if (nf2) hipLaunchKernelGGL((heads_x3_kernel<RT, CT, NCF, 2>), dim3(cdiv(M, 16 * RT), L, branches), dim3(1024), 0, st, p);   \
    else hipLaunchKernelGGL((heads_x3_kernel<RT, CT, 0, 0>), dim3(cdiv(M, 16 * RT), L, branches), dim3(1024), 0, st, p);         \
    break;
#define X3_HEADS_RT(RT)                   \
    switch (ct) {                         \
        case 0: X3_HEADS(RT, 1, 10)       \
        case 1: X3_HEADS(RT, 1, 0)        \
        case 2: X3_HEADS(RT, 2, 0)        \
        case 3: X3_HEADS(RT, 3, 0)        \
        default: X3_HEADS(RT, 4, 0)       \
    }
    // row tiles per block
    if (M <= 512) { X3_HEADS_RT(1) }
    else if (M <= 1024) { X3_HEADS_RT(2) }
    else { X3_HEADS_RT(4) }
#undef X3_HEADS_RT
#undef X3_HEADS
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}

// The RegLayer from either layout.  group_dims is read here, on the host, and travels to the kernel by value (gstart)
int reg_layer_x3_launch(Tables tables, const char* name, const float* outs, const void* const* w, const float* ref, float* reg, int M, int L, int n_fcs,
                        int n_groups, const int* group_dims, const float* pc_range, float dt, const float* dt_rows, void* stream) {
    const bool depth = tables == STACKED;
    X3_CHECK(outs && w && ref && reg && group_dims && pc_range && L > 0 && M >= 0, name, "null pointer or bad size");
    if (depth) X3_CHECK(n_fcs >= 1 && n_fcs <= 3, name, "n_fcs (num_reg_fcs) must be in [1, 3]");
    X3_CHECK(n_groups >= 1 && n_groups <= 10, name, "n_groups must be in [1, 10]");
    unsigned long long gstart = 0;
    int sum = 0;
    for (int g = 0; g < n_groups; ++g) {
        X3_CHECK(group_dims[g] >= 1 && group_dims[g] <= 10, name, "every group_dims entry must be at least 1 (and the sum 10)");
        gstart |= (unsigned long long)sum << (4 * g);
        sum += group_dims[g];
        X3_CHECK(sum <= 10, name, "group_dims must sum to 10, the box code size");
    }
    X3_CHECK(sum == 10, name, "group_dims must sum to 10, the box code size");
    gstart |= 10ull << (4 * n_groups);
    const int nw = depth ? 8 : 11;
    for (int i = 0; i < nw; ++i) X3_CHECK(w[i] != nullptr, name, "null weight");
    if (M == 0) return MV2D_OK;
    RegLayerX3Params p{};
    p.outs = outs; p.reg = reg;
    p.M = M; p.L = L; p.G = n_groups; p.gstart = gstart;
    if (depth) {
        p.n = p.stride = n_fcs;
        stacked(p.s0, p.s1, w[0], w[1], w[2]);
    } else {
        p.n = 2; p.stride = 1;
        p.s0 = X3Layers{(U)w[0], (U)w[1], (Fp)w[2]};
        p.s1 = X3Layers{(U)w[3], (U)w[4], (Fp)w[5]};
    }
    p.t1 = X3Layers{(U)w[nw - 5], (U)w[nw - 4], (Fp)w[nw - 3]};
    p.t2 = (Fp)w[nw - 2]; p.tb2 = (Fp)w[nw - 1];
    p.tail = box_tail(ref, pc_range, dt, dt_rows);
    const hipStream_t st = (hipStream_t)stream;
#define X3_REG_LAYER(RT)                                                                                            \
    if (p.n == 2) hipLaunchKernelGGL((reg_layer_x3_kernel<RT, 2>), dim3(cdiv(M, 16 * RT), L), dim3(1024), 0, st, p);    \
    else hipLaunchKernelGGL((reg_layer_x3_kernel<RT, 0>), dim3(cdiv(M, 16 * RT), L), dim3(1024), 0, st, p);
    // the row-tile rule of heads_x3_launch
    if (M <= 512) { X3_REG_LAYER(1) }
    else if (M <= 1024) { X3_REG_LAYER(2) }
    else { X3_REG_LAYER(4) }
#undef X3_REG_LAYER
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}

}  // namespace

extern "C" int mv2d_heads_fused_x3_nc(const float* outs, const void* const* cls_w, const void* const* reg_w, const float* ref, float* cls,
                                      float* reg, int M, int L, int num_classes, float eps, const float* pc_range, float dt, const float* dt_rows,
                                      void* stream) {
    return heads_x3_launch(PER_LAYER, "mv2d_heads_fused_x3", "mv2d_heads_fused_x3", outs, cls_w, reg_w, ref, cls, reg, M, L, 0, num_classes, eps, pc_range, dt,
                           dt_rows, stream, 2);
}

extern "C" int mv2d_heads_cls_x3_nc(const float* outs, const void* const* cls_w, float* cls, int M, int L, int num_classes, float eps, void* stream) {
    return heads_x3_launch(PER_LAYER, "mv2d_heads_fused_x3", "mv2d_heads_cls_x3", outs, cls_w, nullptr, nullptr, cls, nullptr, M, L, 0, num_classes, eps, nullptr,
                           0.f, nullptr, stream, 1);
}

extern "C" int mv2d_heads_fused_x3(const float* outs, const void* const* cls_w, const void* const* reg_w, const float* ref, float* cls, float* reg,
                                   int M, int L, float eps, const float* pc_range, float dt, const float* dt_rows, void* stream) {
    return mv2d_heads_fused_x3_nc(outs, cls_w, reg_w, ref, cls, reg, M, L, 10, eps, pc_range, dt, dt_rows, stream);
}

extern "C" int mv2d_heads_depth_x3(const float* outs, const void* const* cls_w, const void* const* reg_w, const float* ref, float* cls, float* reg,
                                   int M, int L, int n_fcs, int num_classes, float eps, const float* pc_range, float dt, const float* dt_rows,
                                   void* stream) {
    return heads_x3_launch(STACKED, "mv2d_heads_depth_x3", nullptr, outs, cls_w, reg_w, ref, cls, reg, M, L, n_fcs, num_classes, eps, pc_range, dt, dt_rows,
                           stream, 2);
}

extern "C" int mv2d_heads_cls_depth_x3(const float* outs, const void* const* cls_w, float* cls, int M, int L, int n_fcs, int num_classes, float eps,
                                       void* stream) {
    return heads_x3_launch(STACKED, "mv2d_heads_cls_depth_x3", nullptr, outs, cls_w, nullptr, nullptr, cls, nullptr, M, L, n_fcs, num_classes, eps, nullptr, 0.f,
                           nullptr, stream, 1);
}

extern "C" int mv2d_reg_layer_x3(const float* outs, const void* const* w, const float* ref, float* reg, int M, int L, int n_groups,
                                 const int* group_dims, const float* pc_range, float dt, const float* dt_rows, void* stream) {
    return reg_layer_x3_launch(PER_LAYER, "mv2d_reg_layer_x3", outs, w, ref, reg, M, L, 0, n_groups, group_dims, pc_range, dt, dt_rows, stream);
}

extern "C" int mv2d_reg_layer_depth_x3(const float* outs, const void* const* w, const float* ref, float* reg, int M, int L, int n_fcs, int n_groups,
                                       const int* group_dims, const float* pc_range, float dt, const float* dt_rows, void* stream) {
    return reg_layer_x3_launch(STACKED, "mv2d_reg_layer_depth_x3", outs, w, ref, reg, M, L, n_fcs, n_groups, group_dims, pc_range, dt, dt_rows, stream);
}
