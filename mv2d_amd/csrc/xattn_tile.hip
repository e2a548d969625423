// Cross attention of the MV2D decoder on MFMA tiles, fused with the key / value projections (gfx950 / CDNA4, wave64).
//
// Replaces  kvproj_kernel (K/V of six layers written to HBM) + sparse_xattn_kernel (one VALU dot product per allowed pair)
// for PETRMultiheadAttention's core (MU/petr_transformer.py:426-513, nn.MultiheadAttention with an attn_mask).
//
// The in_proj of the keys / values is folded into the QUERY side, so the key side of every layer and head reads the same two
// key16 row arrays (common.h: fp16 since round 4; Xk = feat + pe, Xv = feat at the gathered positions / RoI cells) and nothing per layer is
// written for the keys:
//
//   logit_h[j] = q_h . (Wk_h x_j + bk_h)      = (Wk_h^T q_h) . x_j + const_h      (const_h cancels in the softmax over j)
//   ctx_h      = sum_j p_hj (Wv_h v_j + bv_h) = Wv_h (sum_j p_hj v_j) + bv_h      (sum_j p_hj = 1)
//
// Three launches per layer:
//   xattn_qmap_kernel    Qt[r] = (Wk_h^T q_h)_h as a 16 x 256 key16 MFMA operand per query: rows 0-7 = the "hi" parts of the
//                        eight heads, rows 8-15 = the "lo" remainders (fp32-class query side), stored fragment-major.  (The map
//                        itself is a bf16x3 product on the fp32 query; only its RESULT is split into the key-side format.)
//   xattn_tile_kernel    one block per query, the keys of its CSR row dealt to the waves in tiles of 16: the tile's Xk rows are
//                        gathered with whole-row (512 B) coalesced loads into an XOR-swizzled LDS tile, logits S[16 x 16] =
//                        Qt . Xk_tile^T on v_mfma_f32_16x16x32_f16 (hi and lo rows of Qt in one instruction: the sum of the
//                        two row groups is the fp32-class logit), online softmax per head, P split hi / lo into the same 16
//                        operand rows, z += P . Xv_tile on v_mfma_f32_16x16x16_f16 with the Xv rows loaded row-contiguous
//                        (16 B per lane) and transposed in registers (v_perm) into key-major B fragments.
//   xattn_ctxmap_kernel  ctx = Wv_h z_h + bv (bf16x3), empty CSR rows -> NaN (the reference's behaviour) or 0.
#include "xattn_walk.h"

namespace {

// ------------------------------------------------------------------------------------------------
// query map: Qt[r][h][s][g][part][e] = part( sum_d q[r][32 h + d] Wk[32 h + d][32 s + 8 g + e] ), part = hi / lo  (operand row n of the
// tile kernel = head n & 7, part n >> 3; one (query, head) = 1 KB contiguous: a wave of this kernel fills whole lines, a fragment load of
// the tile kernel reads 8 whole lines)
// Block = 16 queries, wave = head.  "Swapped" product D[channel][query] so that a lane ends up with 8 CONSECUTIVE channels of one
// query (rows 4g..4g+3 of two channel tiles whose row -> channel assignment is interleaved by the weight packing) = exactly one
// 16-byte chunk of the operand the tile kernel reads.
//   WA_hi / WA_lo [8 heads][16 tiles][64 lanes][8]: lane (m = l & 15, g = l >> 4), e: Wk[32 h + 8 g + e][chan(t, m)],
//   chan(t, m) = 32 (t >> 1) + 8 (m >> 2) + 4 (t & 1) + (m & 3)                                 (ops.pack_xattn_maps)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void xattn_qmap_kernel(const float* __restrict__ q, const uint4* __restrict__ WA_hi,
                                                         const uint4* __restrict__ WA_lo, uint4* __restrict__ Qt, int R) {
    const int lane = threadIdx.x & 63, h = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const int q0 = blockIdx.x * 16;
    const int row = min(q0 + n, R - 1);
    const float* qp = q + (long long)row * C + 32 * h + 8 * g;
    Frag bh, bl;
    split8(*reinterpret_cast<const float4*>(qp), *reinterpret_cast<const float4*>(qp + 4), bh, bl);
    const uint4* wh = WA_hi + (long long)h * 16 * 64 + lane;
    const uint4* wl = WA_lo + (long long)h * 16 * 64 + lane;
    f32x4_t acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        Frag ah, al;
        ah.u = wh[t * 64];
        al.u = wl[t * 64];
        f32x4_t a = {0.f, 0.f, 0.f, 0.f};
        a = mfma_q16_16x16x32(al.v, bh.v, a, 0, 0, 0);
        a = mfma_q16_16x16x32(ah.v, bl.v, a, 0, 0, 0);
        a = mfma_q16_16x16x32(ah.v, bh.v, a, 0, 0, 0);
        acc[t] = a;
    }
    // the wave's 16 rows x 1 KB go through LDS (two halves of 8 rows) so that every store instruction writes ONE row's 1 KB contiguously: the MFMA
    // leaves a lane 32-byte pieces 128 bytes apart (round 3: 18.2 -> 15.3 us for 4800 rows; the kernel is bound by its 39 MB of output, 6.2 us without)
    __shared__ uint4 stage[8][8 * 64];                           // [wave][8 rows x 64 chunks of 16 B], chunk index XOR-ed with the row
    uint4* st = stage[h];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if ((n >> 3) == half) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                Frag hi, lo;
                split8_k16(make_float4(acc[2 * u][0], acc[2 * u][1], acc[2 * u][2], acc[2 * u][3]),
                              make_float4(acc[2 * u + 1][0], acc[2 * u + 1][1], acc[2 * u + 1][2], acc[2 * u + 1][3]), hi, lo);
                const int c = u * 8 + g * 2, r8 = n & 7;
                st[r8 * 64 + (c ^ (r8 << 1))] = hi.u;
                st[r8 * 64 + ((c + 1) ^ (r8 << 1))] = lo.u;
            }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);                      // lgkmcnt(0): the wave's LDS writes have landed
#pragma unroll
        for (int r8 = 0; r8 < 8; ++r8) {
            const int row = q0 + 8 * half + r8;
            const uint4 v = st[r8 * 64 + (lane ^ (r8 << 1))];
            if (row < R) Qt[(long long)row * 512 + h * 64 + lane] = v;
        }
        __builtin_amdgcn_wave_barrier();                         // before the second half overwrites the stage
    }
}

// ------------------------------------------------------------------------------------------------
// context map: ctx[r][32 h + d] = sum_c Wv[32 h + d][c] z[r][h][c] + bv[32 h + d]   (bf16x3: z split hi / lo, Wv split hi / lo)
// Block = 16 queries, wave = head.  WB_hi / WB_lo [8 heads][8 k-steps][2 column tiles][64 lanes][8]:
//   lane (n, g), e: Wv[32 h + 16 nt + n][32 s + 8 g + e]                                          (ops.pack_xattn_maps)
// A CSR row without a key: ctx = NaN (empty_nan, like nn.MultiheadAttention) or 0 — the value bias must not reach such a query.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void xattn_ctxmap_kernel(const float* __restrict__ z, const uint4* __restrict__ WB_hi,
                                                           const uint4* __restrict__ WB_lo, const float* __restrict__ bv,
                                                           const int* __restrict__ row_ptr, float* __restrict__ ctx, int R, int empty_nan) {
    const int lane = threadIdx.x & 63, h = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const int q0 = blockIdx.x * 16;
    const int row = min(q0 + n, R - 1);
    const float* zp = z + ((long long)row * HEADS + h) * C + 8 * g;
    const uint4* wh = WB_hi + (long long)h * 16 * 64 + lane;
    const uint4* wl = WB_lo + (long long)h * 16 * 64 + lane;
    f32x4_t acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float4 x0[8], x1[8];
    {
        // a lane needs 32-byte pieces 128 bytes apart of its row's 1 KB: the rows are read whole (one load instruction = one row's 1 KB) and
        // redistributed through LDS, two halves of 8 rows (chunk index XOR-ed with the row); every lane loading its own pieces from zp was slower
        (void)zp;
        __shared__ float4 stage[8][8 * 64];
        float4* st = stage[h];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float4 v[8];
#pragma unroll
            for (int r8 = 0; r8 < 8; ++r8) {
                const int rr = min(q0 + 8 * half + r8, R - 1);
                v[r8] = *reinterpret_cast<const float4*>(z + ((long long)rr * HEADS + h) * C + 4 * lane);
            }
#pragma unroll
            for (int r8 = 0; r8 < 8; ++r8) st[r8 * 64 + (lane ^ (r8 << 1))] = v[r8];
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);
            if ((n >> 3) == half) {
                const int r8 = n & 7;
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const int c = s * 8 + g * 2;
                    x0[s] = st[r8 * 64 + (c ^ (r8 << 1))];
                    x1[s] = st[r8 * 64 + ((c + 1) ^ (r8 << 1))];
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        Frag ah, al;
        split8(x0[s], x1[s], ah, al);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            Frag bh, bl;
            bh.u = wh[(s * 2 + nt) * 64];
            bl.u = wl[(s * 2 + nt) * 64];
            acc[nt] = mfma_q16_16x16x32(al.v, bh.v, acc[nt], 0, 0, 0);
            acc[nt] = mfma_q16_16x16x32(ah.v, bl.v, acc[nt], 0, 0, 0);
            acc[nt] = mfma_q16_16x16x32(ah.v, bh.v, acc[nt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = q0 + 4 * g + i;
        if (r < R) {
            const bool empty = row_ptr[r + 1] <= row_ptr[r];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int col = 32 * h + 16 * nt + n;
                float v = acc[nt][i] + bv[col];
                if (empty) v = empty_nan ? __uint_as_float(0x7fc00000u) : 0.f;
                ctx[(long long)r * C + col] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// tile attention: see the file header.  One block (NW waves) per query; wave w takes the key tiles w, w + NW, ...
//   Qt  [R][8 heads][8 k-steps][4][hi | lo][8] key16 (xattn_qmap_kernel), Xk / Xv [S][256] key16, CSR row_ptr / col_idx, z [R][8][256] fp32
// LDS (one array): per wave an 8 KB key tile (16 rows x 32 chunks of 16 B, chunk c of row r at slot c ^ (r & 15): the
// fragment reads of 16 different rows hit 16 different bank slots) that later holds the wave's partial z, 512 B of P, and the
// softmax statistics of the merge.
// ------------------------------------------------------------------------------------------------
// XLO, DBG and what a wave does with a tile: XattnWalk (xattn_walk.h)
template <int NW, bool DBG, int XLO>
__global__ __launch_bounds__(64 * NW, 2) void xattn_tile_kernel(const uint4* __restrict__ Qt, const unsigned short* __restrict__ Xk,
                                                             const unsigned short* __restrict__ Xv, const unsigned short* __restrict__ Xk_lo,
                                                             const unsigned short* __restrict__ Xv_lo, const int* __restrict__ row_ptr,
                                                             const int* __restrict__ col_idx, float* __restrict__ z,
                                                             float* __restrict__ dbg_logits, long long dbg_stride, int R, int empty_nan,
                                                             const int* __restrict__ order) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[NW * 8192 + NW * 512 + NW * 64 + (XLO ? NW * 8192 : 0)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, g = lane >> 4;
    // XCD-aware block -> query map (block b runs on XCD b % 8): every XCD gets one contiguous range of queries, so neighbouring
    // queries (T path: overlapping key sets) share an L2.  Speed only; any map is correct.
    int r;
    {
        const int b = blockIdx.x, x = b & 7, qn = R >> 3, rem = R & 7;
        r = (x < rem ? x * (qn + 1) : rem * (qn + 1) + (x - rem) * qn) + (b >> 3);
        // optional query order (T path: the queries of a sample sorted by their smallest key, mv2d_xattn_query_order's perm): blocks that run
        // side by side on an XCD then read overlapping key sets and share its L2.  Speed only.
        if (order) r = order[r];
    }
    const int beg = row_ptr[r], end = row_ptr[r + 1];
    float* zr = z + (long long)r * (HEADS * C);
    if (end <= beg) {
        const float v = empty_nan ? __uint_as_float(0x7fc00000u) : 0.f;
        for (int i = tid; i < HEADS * C; i += 64 * NW) zr[i] = v;
        return;
    }
    float* sst = reinterpret_cast<float*>(smem + NW * 8192 + NW * 512);              // [NW][8] running max, [NW][8] sums
    XattnWalk<XLO, DBG> walk(Xk, Xv, Xk_lo, Xv_lo, lane, beg, end, reinterpret_cast<uint4*>(smem) + wave * 512,
                          reinterpret_cast<uint4*>(smem + NW * 8192 + NW * 512 + NW * 64) + wave * 512,      // XLO: the lo parts of the key tile
                          reinterpret_cast<float*>(smem + NW * 8192) + wave * 128, dbg_logits, dbg_stride);
    walk.reset();
    const int ntile = (end - beg + 15) >> 4;
    if (wave < ntile) {
        const uint4* qp = Qt + (long long)r * 512 + (n & 7) * 64 + g * 2 + (n >> 3);
#pragma unroll
        for (int s = 0; s < 8; ++s) walk.qa[s].u = qp[s * 8];
    }
    int idx_next = wave < ntile ? col_idx[min(beg + 16 * wave + n, end - 1)] : 0;
    for (int tt = wave; tt < ntile; tt += NW) {
        const int myidx = idx_next;
        if (tt + NW < ntile) idx_next = col_idx[min(beg + 16 * (tt + NW) + n, end - 1)];
        typename XattnWalk<XLO, DBG>::VRows v;
        walk.gather(myidx, true, v);
        walk.compute(tt, v);
    }
    // ---- partial (m, l, z) of the wave -> LDS (z into the wave's own key-tile region)
    walk.row_sums();
    if (n == 0 && g < 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sst[wave * 8 + 4 * g + i] = walk.m_run[i];
            sst[NW * 8 + wave * 8 + 4 * g + i] = walk.l_run[i];
        }
    }
    walk.store_z(reinterpret_cast<float*>(smem) + wave * (HEADS * C));
    __syncthreads();
    // ---- merge the waves: thread -> (channel, half of the heads)
    {
        const float* sz = reinterpret_cast<const float*>(smem);
        for (int idx = tid; idx < HEADS * C; idx += 64 * NW) {
            const int h = idx >> 8, c = idx & (C - 1);
            float M = sst[h];
#pragma unroll
            for (int w = 1; w < NW; ++w) M = fmaxf(M, sst[w * 8 + h]);
            float den = 0.f, num = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const float e = __builtin_amdgcn_exp2f(sst[w * 8 + h] - M);        // waves without a tile: 2^(-inf) = 0
                den += sst[NW * 8 + w * 8 + h] * e;
                num += sz[(w * HEADS + h) * C + c] * e;
            }
            zr[h * C + c] = num * __builtin_amdgcn_rcpf(den);
        }
    }
}

}  // namespace

extern "C" int mv2d_xattn_qmap(const float* q, const void* WA_hi, const void* WA_lo, void* Qt, int R, void* stream) {
    MV2D_CHECK_ARG(q && WA_hi && WA_lo && Qt && R >= 0, "mv2d_xattn_qmap: bad args");
    MV2D_CHECK_ARG(((uintptr_t)q & 15) == 0 && ((uintptr_t)WA_hi & 15) == 0 && ((uintptr_t)WA_lo & 15) == 0 && ((uintptr_t)Qt & 15) == 0,
                   "mv2d_xattn_qmap: operands must be 16-byte aligned");
    if (R == 0) return MV2D_OK;
    hipLaunchKernelGGL(xattn_qmap_kernel, dim3(cdiv(R, 16)), dim3(512), 0, (hipStream_t)stream, q, (const uint4*)WA_hi, (const uint4*)WA_lo,
                       (uint4*)Qt, R);
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}

extern "C" int mv2d_xattn_ctxmap(const float* z, const void* WB_hi, const void* WB_lo, const float* bv, const int* row_ptr, float* ctx, int R,
                                 int empty_nan, void* stream) {
    MV2D_CHECK_ARG(z && WB_hi && WB_lo && bv && row_ptr && ctx && R >= 0, "mv2d_xattn_ctxmap: bad args");
    MV2D_CHECK_ARG(((uintptr_t)z & 15) == 0 && ((uintptr_t)WB_hi & 15) == 0 && ((uintptr_t)WB_lo & 15) == 0, "mv2d_xattn_ctxmap: operands must be 16-byte aligned");
    if (R == 0) return MV2D_OK;
    hipLaunchKernelGGL(xattn_ctxmap_kernel, dim3(cdiv(R, 16)), dim3(512), 0, (hipStream_t)stream, z, (const uint4*)WB_hi, (const uint4*)WB_lo, bv,
                       row_ptr, ctx, R, empty_nan);
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}

extern "C" int mv2d_xattn_tile_fwd_ordered(const void* Qt, const void* Xk, const void* Xv, const void* Xk_lo, const void* Xv_lo, const int* row_ptr,
                                           const int* col_idx, float* z, float* dbg_logits, long long dbg_stride, int R, int empty_nan, int waves,
                                           const int* order, int lo_fmt, void* stream);

extern "C" int mv2d_xattn_tile_fwd(const void* Qt, const void* Xk, const void* Xv, const void* Xk_lo, const void* Xv_lo, const int* row_ptr,
                                   const int* col_idx, float* z, float* dbg_logits, long long dbg_stride, int R, int empty_nan, int waves, void* stream) {
    return mv2d_xattn_tile_fwd_ordered(Qt, Xk, Xv, Xk_lo, Xv_lo, row_ptr, col_idx, z, dbg_logits, dbg_stride, R, empty_nan, waves, nullptr, 0, stream);
}

extern "C" int mv2d_xattn_tile_fwd_ordered(const void* Qt, const void* Xk, const void* Xv, const void* Xk_lo, const void* Xv_lo, const int* row_ptr,
                                           const int* col_idx, float* z, float* dbg_logits, long long dbg_stride, int R, int empty_nan, int waves,
                                           const int* order, int lo_fmt, void* stream) {
    MV2D_CHECK_ARG(Qt && Xk && Xv && row_ptr && col_idx && z && R >= 0, "mv2d_xattn_tile_fwd: bad args");
    MV2D_CHECK_ARG(lo_fmt == 0 || (lo_fmt == 1 && Xk_lo), "mv2d_xattn_tile_fwd: lo_fmt is 0 (key16 lo rows) or 1 (e4m3 lo rows; needs the lo rows)");
    MV2D_CHECK_ARG((Xk_lo == nullptr) == (Xv_lo == nullptr), "mv2d_xattn_tile_fwd: Xk_lo and Xv_lo come together");
    MV2D_CHECK_ARG(((uintptr_t)Qt & 15) == 0 && ((uintptr_t)Xk & 15) == 0 && ((uintptr_t)Xv & 15) == 0 && ((uintptr_t)z & 15) == 0 &&
                       ((uintptr_t)Xk_lo & 15) == 0 && ((uintptr_t)Xv_lo & 15) == 0, "mv2d_xattn_tile_fwd: operands must be 16-byte aligned");
    MV2D_CHECK_ARG(waves == 0 || waves == 1 || waves == 2 || waves == 4 || waves == 8, "mv2d_xattn_tile_fwd: waves per query must be 1, 2, 4 or 8 (0: default)");
    if (R == 0) return MV2D_OK;
    const int nw = waves ? waves : 2;      // the engine passes its own choice (2: see engine.py)
#define MV2D_XT(NW, DBG, XLO) hipLaunchKernelGGL((xattn_tile_kernel<NW, DBG, XLO>), dim3(R), dim3(64 * NW), 0, (hipStream_t)stream, (const uint4*)Qt, \
                                                 (const unsigned short*)Xk, (const unsigned short*)Xv, (const unsigned short*)Xk_lo, (const unsigned short*)Xv_lo, \
                                                 row_ptr, col_idx, z, dbg_logits, dbg_stride, R, empty_nan, order)
    // index-exact route (hi + lo rows): two waves per SIMD like the default (round 3: the 312-register build ran one wave per SIMD, 133 us per layer)
    if (Xk_lo && lo_fmt == 1) { if (dbg_logits) MV2D_XT(4, true, 2); else if (nw == 4) MV2D_XT(4, false, 2); else if (nw == 1) MV2D_XT(1, false, 2); else MV2D_XT(2, false, 2); }
    else if (Xk_lo) { if (dbg_logits) MV2D_XT(4, true, 1); else if (nw == 4) MV2D_XT(4, false, 1); else if (nw == 1) MV2D_XT(1, false, 1); else MV2D_XT(2, false, 1); }
    else if (dbg_logits) { if (nw == 8) MV2D_XT(8, true, 0); else if (nw == 2) MV2D_XT(2, true, 0); else if (nw == 1) MV2D_XT(1, true, 0); else MV2D_XT(4, true, 0); }
    else { if (nw == 8) MV2D_XT(8, false, 0); else if (nw == 2) MV2D_XT(2, false, 0); else if (nw == 1) MV2D_XT(1, false, 0); else MV2D_XT(4, false, 0); }
#undef MV2D_XT
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}
