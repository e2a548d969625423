// Building blocks of the row-block kernels (rowblock.hip, branches_x3.hip): a 16-row activation tile that stays in LDS, multiplied by a
// 256x256 weight matrix whose MFMA fragments one wave per 16-column tile holds in registers.
#pragma once
#include "common.h"

namespace {

constexpr int C = 256;

// fp32 tile [16][256]: 4-float chunk c of row r at chunk c ^ r
__device__ __forceinline__ int toff(int row, int col) { return row * C + ((((col >> 2) ^ (row & 15))) << 2) + (col & 3); }

struct Frag { float4 v[16]; };

__device__ __forceinline__ void load_w(Frag& f, const float* __restrict__ W, int ldw, int nrow, int nmax, int fg) {
    const float* wp = W + (long long)min(nrow, nmax - 1) * ldw + 4 * fg;
#pragma unroll
    for (int c = 0; c < 16; ++c) f.v[c] = *reinterpret_cast<const float4*>(wp + 16 * c);
}

__device__ __forceinline__ f32x4_t tile_mma(const float* __restrict__ As, const Frag& f, int fr, int fg) {
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const float4 a = *reinterpret_cast<const float4*>(As + fr * C + (((4 * c + fg) ^ fr) << 2));
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, f.v[c].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, f.v[c].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, f.v[c].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, f.v[c].w, acc, 0, 0, 0);
    }
    return acc;
}

typedef q16x8_t mfma_bf16x8;      // the query side's 16-bit split format (common.h "q16": fp16 pairs since round 5)
union BFrag { uint4 u; mfma_bf16x8 v; };

__device__ __forceinline__ void split4(const float4& v, uint2& hi, uint2& lo) {
    split_q16x4(v, hi, lo);
}

// one 16x16 tile: sum over 8 k-steps of a_hi.w_hi + a_lo.w_hi + a_hi.w_lo; activation rows from the bf16 LDS images (512 B rows,
// 16-byte chunk c of row r at c ^ r), weight fragments (hi, lo) already in registers
__device__ __forceinline__ f32x4_t tile_mma_x3(const unsigned char* __restrict__ ah, const unsigned char* __restrict__ al, const BFrag wh[8],
                                               const BFrag wl[8], int fr, int fg) {
    f32x4_t a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        BFrag xh, xl;
        const int off = fr * 512 + (((4 * s + fg) ^ fr) << 4);
        xh.u = *reinterpret_cast<const uint4*>(ah + off);
        xl.u = *reinterpret_cast<const uint4*>(al + off);
        a0 = mfma_q16_16x16x32(xh.v, wh[s].v, a0, 0, 0, 0);
        a1 = mfma_q16_16x16x32(xl.v, wh[s].v, a1, 0, 0, 0);
        a1 = mfma_q16_16x16x32(xh.v, wl[s].v, a1, 0, 0, 0);
    }
    return f32x4_t{a0[0] + a1[0], a0[1] + a1[1], a0[2] + a1[2], a0[3] + a1[3]};
}

__device__ __forceinline__ void load_w_x3(BFrag wh[8], BFrag wl[8], const unsigned short* __restrict__ Wh, const unsigned short* __restrict__ Wl,
                                          int tile, int lane) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {                 // fragment-major [k-step][16 column tiles][lane][8]
        const long long o = (((long long)s * 16 + tile) * 64 + lane) * 8;
        wh[s].u = *reinterpret_cast<const uint4*>(Wh + o);
        wl[s].u = *reinterpret_cast<const uint4*>(Wl + o);
    }
}

// load_w_x3 with the matrix as a UNIFORM base and the lane's part of the address ((16-column tile, lane) of a k-step: 8 * threadIdx.x with one
// wave per tile) as one 32-bit offset: the sixteen 64-bit per-lane addresses of load_w_x3 (32 VGPRs next to the 64 of the fragments) make a
// kernel with four row tiles per block spill, this form keeps one
__device__ __forceinline__ void load_w_x3_uniform(BFrag wh[8], BFrag wl[8], const unsigned short* __restrict__ Wh, const unsigned short* __restrict__ Wl,
                                                  unsigned lane_off) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {                 // fragment-major [k-step][16 column tiles][lane][8]
        wh[s].u = *reinterpret_cast<const uint4*>(Wh + s * (16 * 64 * 8) + lane_off);
        wl[s].u = *reinterpret_cast<const uint4*>(Wl + s * (16 * 64 * 8) + lane_off);
    }
}

// LayerNorm of one 256-wide row held 4 values per lane (columns c0 .. c0 + 3), the row spread over one wave
__device__ __forceinline__ float4 ln_row(float4 v, const float* __restrict__ w, const float* __restrict__ b, int c0, float eps) {
    const float mean = wave_sum(v.x + v.y + v.z + v.w) * (1.0f / C);
    const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
    const float var = wave_sum(dx * dx + dy * dy + dz * dz + dw * dw) * (1.0f / C);
    const float rstd = 1.0f / sqrtf(var + eps);
    const float4 ww = *reinterpret_cast<const float4*>(w + c0), bb = *reinterpret_cast<const float4*>(b + c0);
    return make_float4(dx * rstd * ww.x + bb.x, dy * rstd * ww.y + bb.y, dz * rstd * ww.z + bb.z, dw * rstd * ww.w + bb.w);
}

// The tail of the regression branch on column o of row m of the raw box code (cross_attention_head.py:219-238: add inverse_sigmoid(ref) to
// (cx, cy) and cz, sigmoid, de-normalise; T head: velocity / dt, mv2d_t_head.py:136-140).  pd = pc_range[3:] - pc_range[:3]; dt_rows
// (optional, [M]: a batch of samples) overrides dt
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

inline BoxTail box_tail(const float* ref, const float* pc_range, float dt, const float* dt_rows) {
    return BoxTail{ref, pc_range[0], pc_range[1], pc_range[2], pc_range[3] - pc_range[0], pc_range[4] - pc_range[1], pc_range[5] - pc_range[2],
                   dt, dt_rows};
}

}  // namespace
