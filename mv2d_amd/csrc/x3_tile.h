// Building blocks of the row-block kernels (rowblock.hip, reglayer.hip): a 16-row activation tile that stays in LDS, multiplied by a
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

}  // namespace
