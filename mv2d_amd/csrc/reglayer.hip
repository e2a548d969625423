// The regression branch of a decoder layer as the reference's RegLayer (RH/bbox_heads/cross_attention_head.py:52-83, the head's
// use_reg_layer switch), fused with the box-code tail of heads_fused_x3_kernel's branch 1 (rowblock.hip):
//
//   reg_feat = ReLU(L2(ReLU(L1(x))))                               two shared Linear(256,256) + ReLU
//   h_g      = ReLU(T1_g(reg_feat)),  out[:, cols of g] = T2_g(h_g)    one Linear(256,256) + ReLU + Linear(256,d_g) per group g
//   out      -> + inverse_sigmoid(ref) on (cx, cy) and cz, sigmoid, pc_range; velocity / dt         (:216-238, mv2d_t_head.py:136-140)
//
// One block of 16 waves owns RT row tiles (16 rows each) of one layer and runs the 2 + G linears on them: wave w computes column tile w of a
// linear (bf16x3 on v_mfma_f32_16x16x32, fragments of the NEXT matrix in flight behind the current one) and owns row w of every tile in the
// row stages.  reg_feat stays in the hi / lo LDS images for all G task heads; h_g goes through the fp32 tile, and the group's d_g output
// columns are exact fp32 dot products of the row with the rows of T2 (staged in LDS once: [10][256]), reduced over the wave -- so the
// output layer costs d_g wave reductions per row instead of one 64-MFMA chain per group on a single wave.
// LDS: 32 KB per row tile + 10 KB (138 KB at RT = 4).
#include "x3_tile.h"

namespace {

struct RegLayerParams {
    const float* outs;
    const unsigned short* s1h; const unsigned short* s1l; const float* sb1;      // shared layer 1: [L] fragment-major hi / lo, bias [L,256]
    const unsigned short* s2h; const unsigned short* s2l; const float* sb2;      // shared layer 2
    const unsigned short* t1h; const unsigned short* t1l; const float* tb1;      // task heads, first layers: [L][G]
    const float* t2; const float* tb2;                                           // second layers: [L][10][256] (row o: the group of column o), [L][10]
    const float* ref; float* reg;
    int M, L, G;
    unsigned long long gstart;            // 4 bits per group boundary: columns of group g = [nib(g), nib(g + 1)), nib(G) = 10
    float pc0, pc1, pc2, pd0, pd1, pd2, dt; const float* dt_rows;
};

// load_w_x3 with the matrix as a UNIFORM base and the lane's part of the address as one 32-bit offset: the sixteen 64-bit per-lane addresses
// of load_w_x3 (32 VGPRs next to the 64 of the fragments) make the RT = 4 instance of this kernel spill ~100 registers, this form keeps one
__device__ __forceinline__ void load_w_x3_uniform(BFrag wh[8], BFrag wl[8], const unsigned short* __restrict__ Wh, const unsigned short* __restrict__ Wl,
                                                  unsigned lane_off) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {                 // fragment-major [k-step][16 column tiles][lane][8]
        wh[s].u = *reinterpret_cast<const uint4*>(Wh + s * (16 * 64 * 8) + lane_off);
        wl[s].u = *reinterpret_cast<const uint4*>(Wl + s * (16 * 64 * 8) + lane_off);
    }
}

template <int RT>
__global__ __launch_bounds__(1024) void reg_layer_x3_kernel(RegLayerParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char ah[RT * 16 * 512], al[RT * 16 * 512];
    __shared__ __attribute__((aligned(16))) float tb[RT * 16 * C];
    __shared__ __attribute__((aligned(16))) float w2s[10 * C];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
    // the row blocks of one layer run on ONE XCD (see heads_fused_x3_kernel)
    const int lin = xcd_chunked(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
    const int mb = (lin % gridDim.x) * (16 * RT), l = lin / gridDim.x;
    const long long wo = (long long)l * C * C, bl = (long long)l * C;
    float4 av[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t)
        av[t] = *reinterpret_cast<const float4*>(p.outs + ((long long)l * p.M + min(mb + 16 * t + wave, p.M - 1)) * C + lane * 4);
    const unsigned woff = (unsigned)tid * 8u;                           // (16-column tile = wave, lane) in a k-step of a fragment-major matrix
    BFrag wh[8], wl[8];
    load_w_x3_uniform(wh, wl, p.s1h + wo, p.s1l + wo, woff);
    if (tid < 10 * C / 4) *reinterpret_cast<float4*>(w2s + 4 * tid) = *reinterpret_cast<const float4*>(p.t2 + (long long)l * 10 * C + 4 * tid);
    const int aoff = wave * 512 + (((lane >> 1) ^ wave) << 4) + (lane & 1) * 8;     // this thread's 4 values in the bf16 images of a tile
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
    f32x4_t acc[RT];
    // ---- the two shared layers: linear -> ReLU -> hi / lo images
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t] = tile_mma_x3(ah + t * 8192, al + t * 8192, wh, wl, fr, fg);
        __builtin_amdgcn_sched_barrier(0);              // the fragments are dead here: the next matrix reuses their registers
        // in flight during the row stage: shared layer 2, then the first task head
        if (s == 0) load_w_x3_uniform(wh, wl, p.s2h + wo, p.s2l + wo, woff);
        else load_w_x3_uniform(wh, wl, p.t1h + wo * p.G, p.t1l + wo * p.G, woff);
        {
            const float b = (s == 0 ? p.sb1 : p.sb2)[bl + col];
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
    for (int g = 0; g < p.G; ++g) {
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t] = tile_mma_x3(ah + t * 8192, al + t * 8192, wh, wl, fr, fg);
        __builtin_amdgcn_sched_barrier(0);
        if (g + 1 < p.G) {
            const long long wg = (wo * p.G) + (long long)(g + 1) * C * C;
            load_w_x3_uniform(wh, wl, p.t1h + wg, p.t1l + wg, woff);
        }
        const float b = p.tb1[(bl * p.G) + g * C + col];
        if (g > 0) __syncthreads();                                     // the row stage of group g - 1 has read the tile
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) tb[t * 16 * C + toff(4 * fg + r, col)] = acc[t][r] + b;
        __syncthreads();
        const int o0 = (int)((p.gstart >> (4 * g)) & 15), o1 = (int)((p.gstart >> (4 * g + 4)) & 15);
        float4 v[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            const float4 x = *reinterpret_cast<float4*>(trow + t * 16 * C);
            v[t] = make_float4(relu_f(x.x), relu_f(x.y), relu_f(x.z), relu_f(x.w));
        }
        for (int o = o0; o < o1; ++o) {
            const float4 w = *reinterpret_cast<const float4*>(w2s + o * C + 4 * lane);
#pragma unroll
            for (int t = 0; t < RT; ++t) {                              // RT independent reductions side by side
                const float s = wave_sum((v[t].x * w.x + v[t].y * w.y) + (v[t].z * w.z + v[t].w * w.w));
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
        float v = outv[t] + b2;
        // cross_attention_head.py:219-238: add inverse_sigmoid(ref) to (cx, cy) and cz, sigmoid, de-normalise; T head: v / dt
        if (lane == 0 || lane == 1 || lane == 4) {
            const int k = lane == 4 ? 2 : lane;
            const float x = fminf(fmaxf(p.ref[m * 3 + k], 0.f), 1.f);
            const float is = logf(fmaxf(x, 1e-5f) / fmaxf(1.f - x, 1e-5f));
            const float sg = 1.f / (1.f + expf(-(v + is)));
            v = lane == 0 ? sg * p.pd0 + p.pc0 : (lane == 1 ? sg * p.pd1 + p.pc1 : sg * p.pd2 + p.pc2);
        } else if (lane >= 8) {
            const float dt = p.dt_rows ? p.dt_rows[m] : p.dt;
            if (dt != 0.f) v = v / dt;
        }
        p.reg[((long long)l * p.M + m) * 10 + lane] = v;
    }
}

}  // namespace

extern "C" int mv2d_reg_layer_x3(const float* outs, const void* const* w, const float* ref, float* reg, int M, int L, int n_groups,
                                 const int* group_dims, const float* pc_range, float dt, const float* dt_rows, void* stream) {
    // w: {s1_hi,s1_lo,s1_b, s2_hi,s2_lo,s2_b, t1_hi,t1_lo,t1_b, t2_w,t2_b} device pointers (include/mv2d_hip.h); group_dims is read here, on
    // the host, and travels to the kernel by value
    MV2D_CHECK_ARG(outs && w && ref && reg && group_dims && pc_range && L > 0 && M >= 0, "mv2d_reg_layer_x3: null pointer or bad size");
    MV2D_CHECK_ARG(n_groups >= 1 && n_groups <= 10, "mv2d_reg_layer_x3: n_groups must be in [1, 10]");
    unsigned long long gstart = 0;
    int sum = 0;
    for (int g = 0; g < n_groups; ++g) {
        MV2D_CHECK_ARG(group_dims[g] >= 1 && group_dims[g] <= 10, "mv2d_reg_layer_x3: every group_dims entry must be at least 1 (and the sum 10)");
        gstart |= (unsigned long long)sum << (4 * g);
        sum += group_dims[g];
        MV2D_CHECK_ARG(sum <= 10, "mv2d_reg_layer_x3: group_dims must sum to 10, the box code size");
    }
    MV2D_CHECK_ARG(sum == 10, "mv2d_reg_layer_x3: group_dims must sum to 10, the box code size");
    gstart |= 10ull << (4 * n_groups);
    for (int i = 0; i < 11; ++i) MV2D_CHECK_ARG(w[i] != nullptr, "mv2d_reg_layer_x3: null weight");
    if (M == 0) return MV2D_OK;
    typedef const unsigned short* U; typedef const float* Fp;
    RegLayerParams p{outs, (U)w[0], (U)w[1], (Fp)w[2], (U)w[3], (U)w[4], (Fp)w[5], (U)w[6], (U)w[7], (Fp)w[8], (Fp)w[9], (Fp)w[10],
                     ref, reg, M, L, n_groups, gstart,
                     pc_range[0], pc_range[1], pc_range[2], pc_range[3] - pc_range[0], pc_range[4] - pc_range[1], pc_range[5] - pc_range[2], dt, dt_rows};
    const hipStream_t st = (hipStream_t)stream;
    // the row-tile rule of mv2d_heads_fused_x3_nc
    if (M <= 512) hipLaunchKernelGGL((reg_layer_x3_kernel<1>), dim3(cdiv(M, 16), L), dim3(1024), 0, st, p);
    else if (M <= 1024) hipLaunchKernelGGL((reg_layer_x3_kernel<2>), dim3(cdiv(M, 32), L), dim3(1024), 0, st, p);
    else hipLaunchKernelGGL((reg_layer_x3_kernel<4>), dim3(cdiv(M, 64), L), dim3(1024), 0, st, p);
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}
