// Building blocks of the cross-attention kernels (xattn_tile.hip, xattn_fused.hip, xattn_group.hip): the fragment types and split helpers of all
// three, and XattnWalk -- what ONE WAVE does with ONE 16-key tile of a query's CSR row.  xattn_tile_kernel and phase B of xattn_fused_kernel are
// this walk with their own loop around it, which is why the fused kernel is bit for bit the three kernels with one wave per query
// (tests/test_gpu_kernels.py::test_xattn_fused_equals_the_three_kernels -- one piece of code against itself, no evidence for the walk).
// The walk's reference check is tests/test_gpu_xattn_lo.py: logits, z and ctx of every row against fp64 with hi rows alone, key16 lo and e4m3 lo
// rows, on rows of 0 .. 613 keys at the edges of the tile and of 1, 2, 4, 8 waves, and on rows whose hi halves are identical, where the
// lo terms carry all of the result (tests/xattn_cases.py).  xattn_group.hip takes only the small helpers; its own walk is held there too.
#pragma once
#include "common.h"
#include <type_traits>

namespace {

constexpr int C = 256, HEADS = 8;
constexpr float LOG2E = 1.4426950408889634f;

typedef q16x8_t q16x8;                  // the maps run in the query side's split format (common.h "q16": fp16 pairs since round 5)
union Frag { uint4 u; q16x8 v; };
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));      // staging registers (arrays of HIP's uint4 STRUCT that live across a loop end up in scratch)
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// fp32 x 8 -> q16 hi / lo fragments (the operands of the query and context maps)
__device__ __forceinline__ void split8(const float4& x0, const float4& x1, Frag& hi, Frag& lo) {
    const float f[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    unsigned int h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split_q16x2(f[2 * i], f[2 * i + 1], h[i], l[i]);
    hi.u = make_uint4(h[0], h[1], h[2], h[3]);
    lo.u = make_uint4(l[0], l[1], l[2], l[3]);
}
// fp32 x 8 -> key16 hi / lo fragments (the format the tile MFMAs read)
__device__ __forceinline__ void split8_k16(const float4& x0, const float4& x1, Frag& hi, Frag& lo) {
    const float f[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    unsigned int h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split_k16x2(f[2 * i], f[2 * i + 1], h[i], l[i]);
    hi.u = make_uint4(h[0], h[1], h[2], h[3]);
    lo.u = make_uint4(l[0], l[1], l[2], l[3]);
}

// (v_perm_b32: bytes 0-3 of the selector index {S1 = a: 0..3, S0 = b: 4..7}; the shift / mask formulation compiled to two VALU ops per pair)
__device__ __forceinline__ unsigned int lo_pair(unsigned int a, unsigned int b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }     // (a.lo16, b.lo16)
__device__ __forceinline__ unsigned int hi_pair(unsigned int a, unsigned int b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }     // (a.hi16, b.hi16)

// maximum over the 16 lanes of a DPP row (lane & 15 = the key of a tile): two quad permutes, then the half-row and the row mirror.  Four
// v_max with a DPP operand instead of four dependent ds_bpermute round trips per softmax row.
#define XATTN_DPP(v, ctrl) __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), ctrl, 0xF, 0xF, true))
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, XATTN_DPP(v, 0xB1));      // quad_perm [1,0,3,2]
    v = fmaxf(v, XATTN_DPP(v, 0x4E));      // quad_perm [2,3,0,1]
    v = fmaxf(v, XATTN_DPP(v, 0x141));     // row_half_mirror
    v = fmaxf(v, XATTN_DPP(v, 0x140));     // row_mirror
    return v;
}

// ------------------------------------------------------------------------------------------------
// One wave, one query, one key tile at a time.
//   Xk / Xv [S][256] key16 rows; CSR row [beg, end) of the query; qa = the query's Qt operand (xattn_qmap_kernel's layout: operand row n = head
//   n & 7, part n >> 3), loaded by the caller.  LDS of the wave: kt = an 8 KB key tile (16 rows x 32 chunks of 16 B, chunk c of row r at slot
//   c ^ (r & 15): the fragment reads of 16 different rows hit 16 different bank slots), kt2 = the same for the lo parts (XLO), pl = 512 B of P.
//   XLO: 0 = key16 rows alone (default route); the engine's index-exact route brings the key / value rows as hi + lo pairs (fp32-class key side):
//   logits += Qt_hi . Xk_lo, z += P_hi . Xv_lo (the lo x lo terms, 2^-18 relative, are dropped) -- 1 = key16 lo rows, 2 = e4m3 lo rows (common.h
//   "lo8": 256-byte rows, converted to key16 in registers on their way into the LDS tile / the v_perm transposes -- the MFMAs and everything
//   behind them are those of XLO = 1).  DBG: the logits of the valid pairs are also written to dbg_logits[head][pair].
// A tile is gather() (with_k = false when the caller has brought the key rows itself: request_k / stage_k) and compute(); after the last tile
// row_sums() and store_z().  The KEY INDICES of a tile (`myidx`: lane (n, *) holds the index of key n) the caller requests one tile AHEAD
// (round 4: a tile is two dependent round trips, index then rows; the index trip of the next tile runs under the current tile's gather and
// arithmetic: cfg3_t 94.5 -> 87.3 us per layer).
// ------------------------------------------------------------------------------------------------
// LO8B (XLO = 2 only; the fused kernel): the lo key tile in LDS keeps the e4m3 BYTES (16 rows x 32 chunks of 8 B = 4 KB, chunk c of row r at slot
// c ^ 2 r: the 8-byte fragment reads of a half wave -- 16 rows x 2 chunks -- hit 32 different bank pairs) and compute() widens them with the same
// lo8_chunk as it reads the fragment: the same conversion of the same bytes, as many per lane and tile, on 12 KB of LDS per wave instead of 16.
// LO8B is the fused kernel above 8 queries per block: three waves per SIMD, i.e. 168 registers per lane and no scratch.  Same arithmetic in the same
// order; what also changes is what lives across the tile loop and when the lo value rows are requested (see fresh(), compute()).
template <int XLO, bool DBG, bool LO8B = false>
struct XattnWalk {
    static_assert(!LO8B || XLO == 2, "LO8B: the e4m3 lo rows only");
    typedef std::conditional_t<XLO == 2, u32x2, u32x4> lo_t;      // a lane's piece of a lo row: 16 bytes of key16, 8 of e4m3
    struct KRows { u32x4 hi[8]; lo_t lo[XLO ? 8 : 1]; };          // staging of a tile's key rows
    struct VRows { u32x4 hi[4][2]; lo_t lo[XLO ? 4 : 1][2]; };    // a tile's value rows: they stay in registers

    const unsigned short *Xk, *Xv, *Xk_lo, *Xv_lo;
    int lane, n, g;
    int beg, end;
    uint4 *kt, *kt2;
    float* pl;
    float* dbg_logits;
    long long dbg_stride;
    // this lane's rows of S / z: operand rows 4g + i; rows 0-7 carry the hi parts, 8-15 the lo parts of head (4 (g & 1) + i)
    Frag qa[8];
    float m_run[4], l_run[4];
    f32x4_t Z[16];

    __device__ __forceinline__ XattnWalk(const unsigned short* Xk_, const unsigned short* Xv_, const unsigned short* Xk_lo_, const unsigned short* Xv_lo_,
                                         int lane_, int beg_, int end_, uint4* kt_, uint4* kt2_, float* pl_, float* dbg_logits_ = nullptr,
                                         long long dbg_stride_ = 0)
        : Xk(Xk_), Xv(Xv_), Xk_lo(Xk_lo_), Xv_lo(Xv_lo_), lane(lane_), n(lane_ & 15), g(lane_ >> 4), beg(beg_), end(end_), kt(kt_), kt2(kt2_), pl(pl_),
          dbg_logits(dbg_logits_), dbg_stride(dbg_stride_) {}

    // LO8B: the lane's constants are made opaque once per use, so that the ~55 LDS / gather addresses
    // derived from them are recomputed per tile (two VALU operations each) and do not live across the tile loop as registers -- hipcc hoisted them and spilled.
    __device__ __forceinline__ static int fresh(int x) {
        if constexpr (LO8B) asm volatile("" : "+v"(x));
        return x;
    }
    // the value of lane `src` (0 .. 63): LO8B spares __shfl's own lane arithmetic and the register it keeps
    __device__ __forceinline__ static int shfl(int v, int src) {
        if constexpr (LO8B) return __builtin_amdgcn_ds_bpermute(src << 2, v);
        else return __shfl(v, src, 64);
    }
    __device__ __forceinline__ void relane() {
        lane = fresh(lane);
        n = lane & 15;
        g = lane >> 4;
    }

    __device__ __forceinline__ void reset() {
#pragma unroll
        for (int i = 0; i < 4; ++i) { m_run[i] = -INFINITY; l_run[i] = 0.f; }
#pragma unroll
        for (int u = 0; u < 16; ++u) Z[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }

    // ---- the pieces of a gather: Xk rows whole (lanes 0-31 one row, 32-63 the next), Xv rows as 16-byte column chunks of keys 4g..4g+3
    // (byte offsets as 32-bit unsigned: scalar base + vector offset addressing instead of 64-bit address arithmetic per row;
    //  the row arrays must stay below 4 GB = 2^23 rows of 512 B, include/mv2d_hip.h)
    __device__ __forceinline__ void load_v(const unsigned short* V_, int myidx, u32x4 (&dst)[4][2]) const {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned int vidx = (unsigned int)shfl(myidx, 4 * g + e);
            const char* vp = reinterpret_cast<const char*>(V_) + ((vidx << 9) + 16u * (unsigned)n);
            dst[e][0] = *reinterpret_cast<const u32x4*>(vp);
            dst[e][1] = *reinterpret_cast<const u32x4*>(vp + 256);
        }
    }
    __device__ __forceinline__ void load_k(const unsigned short* K_, int myidx, u32x4 (&dst)[8]) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned int ridx = (unsigned int)shfl(myidx, 2 * i + (lane >> 5));
            dst[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(K_) + ((ridx << 9) + (unsigned)(lane & 31) * 16u));
        }
    }
    __device__ __forceinline__ void store_k(uint4* tile, const u32x4 (&src)[8]) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int rowi = 2 * i + (lane >> 5);
            reinterpret_cast<u32x4*>(tile)[rowi * 32 + ((lane & 31) ^ (rowi & 15))] = src[i];
        }
    }
    // e4m3 lo rows: the same lane -> (row, channels) assignment at half the bytes (8 per lane and row: a half wave reads one 256-byte row)
    __device__ __forceinline__ void load_v8(const unsigned short* V_, int myidx, u32x2 (&dst)[4][2]) const {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned int vidx = (unsigned int)shfl(myidx, 4 * g + e);
            const char* vp = reinterpret_cast<const char*>(V_) + ((vidx << 8) + 8u * (unsigned)n);
            dst[e][0] = *reinterpret_cast<const u32x2*>(vp);
            dst[e][1] = *reinterpret_cast<const u32x2*>(vp + 128);
        }
    }
    __device__ __forceinline__ void load_k8(const unsigned short* K_, int myidx, u32x2 (&dst)[8]) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned int ridx = (unsigned int)shfl(myidx, 2 * i + (lane >> 5));
            dst[i] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const char*>(K_) + ((ridx << 8) + (unsigned)(lane & 31) * 8u));
        }
    }
    __device__ __forceinline__ void store_k8(uint4* tile, const u32x2 (&src)[8]) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int rowi = 2 * i + (lane >> 5);
            if constexpr (LO8B) reinterpret_cast<u32x2*>(tile)[rowi * 32 + ((lane & 31) ^ (2 * rowi))] = src[i];
            else tile[rowi * 32 + ((lane & 31) ^ (rowi & 15))] = lo8_chunk(make_uint2(src[i].x, src[i].y));
        }
    }
    // the hi and lo halves of the 16 key rows are requested together (16 loads in flight) ...
    __device__ __forceinline__ void request_k(int myidx, KRows& k) {
        if constexpr (LO8B) relane();
        load_k(Xk, myidx, k.hi);
        if constexpr (XLO == 1) load_k(Xk_lo, myidx, k.lo);
        if constexpr (LO8B) relane();
        if constexpr (XLO == 2) load_k8(Xk_lo, myidx, k.lo);
    }
    // ... and go to the LDS tile
    __device__ __forceinline__ void stage_k(const KRows& k) {
        if constexpr (LO8B) relane();
        store_k(kt, k.hi);
        if constexpr (XLO == 1) store_k(kt2, k.lo);
        if constexpr (LO8B) relane();
        if constexpr (XLO == 2) store_k8(kt2, k.lo);
    }
    __device__ __forceinline__ void request_v(int myidx, VRows& v) const {
        load_v(Xv, myidx, v.hi);
        if constexpr (XLO == 1) load_v(Xv_lo, myidx, v.lo);
        if constexpr (XLO == 2) load_v8(Xv_lo, myidx, v.lo);
    }

    // The rows of tile `myidx`.  Index-exact route, TWO PHASES per tile (round 4): the key rows first; only when they are in LDS the hi and lo value
    // rows are requested -- into the registers the key rows just left -- and arrive while the logits and the softmax run.  (Round 3 requested
    // K hi, V hi up front and the lo halves behind the first LDS writes, in 32 more registers: 314 us instead of 92 us per layer at cfg3_t for
    // twice the bytes.)  The e4m3 lo halves (round 6) are 8-byte loads and 16 + 16 staging registers in the same order.
    // Requesting the ROWS of the next tile ahead as well (software pipelining: key rows through a second register set, or key + value rows with
    // two named value buffers, 230 / 256 registers) does not pay: cfg3_t 89.9 -> 87.9 / 91.3 us, cfg5_t 85.0 -> 81.8 / 84.6, cfg2_s 63.2 ->
    // 66.3 / 68.2 (same box, round 4) -- twice the bytes in flight per wave buy nothing, the kernel sits at what the memory system delivers
    // for 512-byte rows (4-5 TB/s from HBM, 10-12 TB/s where L2 serves the repeats), not at a per-wave latency chain.  The same for the fused
    // kernel with e4m3 lo rows in round 6 (110.6 against 98.6 us per cfg2_s launch: profiles/r06_xattn_fused_lo8_experiments.txt, 1).
    __device__ __forceinline__ void gather(int myidx, bool with_k, VRows& v) {
        if constexpr (XLO != 0) {
            if (with_k) {
                KRows k;
                request_k(myidx, k);
                stage_k(k);
            }
            if constexpr (LO8B) {
                relane();
                load_v(Xv, myidx, v.hi);
            } else {
                request_v(myidx, v);
            }
        } else if (with_k) {
            KRows k;
            request_k(myidx, k);
            request_v(myidx, v);
            stage_k(k);
        } else {
            request_v(myidx, v);
        }
        __builtin_amdgcn_wave_barrier();
    }

    // logits, online softmax and P . V of tile tt: the key tile is in LDS (kt, XLO: kt2), the value rows in registers
    // (LO8B: gather() has requested the hi value rows only; the lo rows of the tile's keys `myidx` are requested here, behind the logits MFMAs -- 16 registers)
    __device__ __forceinline__ void compute(int tt, VRows& v, int myidx = 0) {
        const int kbase = beg + 16 * tt;
        if constexpr (LO8B) relane();
        // ---- logits of the tile: D[row 4g+i][key n] = sum_c Qt[row][c] Xk[key][c]
        f32x4_t sacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            Frag kb;
            kb.u = kt[n * 32 + ((4 * s + g) ^ n)];
            sacc = mfma_k16_16x16x32(qa[s].u, kb.u, sacc);
            if (XLO) {
                Frag kl, qh;
                if constexpr (LO8B) kl.u = lo8_chunk(reinterpret_cast<const uint2*>(kt2)[n * 32 + ((4 * s + g) ^ (2 * n))]);
                else kl.u = kt2[n * 32 + ((4 * s + g) ^ n)];
                qh.u = n < 8 ? qa[s].u : make_uint4(0u, 0u, 0u, 0u);              // hi rows only
                sacc = mfma_k16_16x16x32(qh.u, kl.u, sacc);
            }
        }
        if constexpr (LO8B) {
            __builtin_amdgcn_sched_barrier(0);
            relane();
            load_v8(Xv_lo, myidx, v.lo);
            __builtin_amdgcn_sched_barrier(0);
        }
        const bool valid = kbase + n < end;
        float sv[4], p[4], alpha[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // hi rows + lo rows (head 4 (g & 1) + i) sit 32 lanes apart: one v_permlane32_swap instead of a trip through the LDS crossbar
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(sacc[i]), __float_as_uint(sacc[i]), false, false);
            const float full = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
            if (DBG && dbg_logits && g < 2 && valid) dbg_logits[(long long)(4 * g + i) * dbg_stride + kbase + n] = full;
            sv[i] = valid ? full * LOG2E : -INFINITY;                               // the softmax runs in base 2 (v_exp_f32)
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float tm = sv[i];
            tm = row16_max(tm);                                                      // over the 16 key lanes, DPP (no LDS round trips)
            const float m_new = fmaxf(m_run[i], tm);
            alpha[i] = __builtin_amdgcn_exp2f(m_run[i] - m_new);
            p[i] = __builtin_amdgcn_exp2f(sv[i] - m_new);
            l_run[i] = l_run[i] * alpha[i] + p[i];                                   // per-lane share of the row sum (reduced at the end)
            m_run[i] = m_new;
        }
        // ---- P as the A operand of the 16x16x16 MFMA: lane (row n, g): keys 4g..4g+3 of head n & 7, hi (n < 8) or lo part
        if (g < 2) {
#pragma unroll
            for (int i = 0; i < 4; ++i) pl[(4 * g + i) * 16 + n] = p[i];
        }
        __builtin_amdgcn_wave_barrier();
        uint2 pa, pah;
        {
            const float4 pv = *reinterpret_cast<const float4*>(pl + (n & 7) * 16 + 4 * g);
            unsigned int h0, h1, l0, l1;
            split_k16x2_bounded(pv.x, pv.y, h0, l0);                               // probabilities: inside the fp16 range, no clamp
            split_k16x2_bounded(pv.z, pv.w, h1, l1);
            pa = n < 8 ? make_uint2(h0, h1) : make_uint2(l0, l1);
            pah = n < 8 ? make_uint2(h0, h1) : make_uint2(0u, 0u);
        }
        // ---- z = alpha z + P . Xv_tile; column tile (H, w): output column n <-> channel 128 H + 8 n + w
        // The rescaling runs unconditionally.  In the first tile of a wave alpha = 2^-inf = 0 multiplies rows that are still 0; a guard `if (not the
        // first tile)` is wave-uniform but not provably so and compiled to 64 v_cndmask per tile (a quarter of the loop's vector instructions:
        // 65 -> 60 us per cfg2_s layer without it).  Skipping the 64 multiplications behind a ballot when no head's maximum moved is exact but
        // slower (61.3 -> 62.2 us: the branch costs more than the multiplications it saves).
#pragma unroll
        for (int u = 0; u < 16; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) Z[u][i] *= alpha[i];
#pragma unroll
        for (int H = 0; H < 2; ++H) {
            const unsigned int r0[4] = {v.hi[0][H].x, v.hi[0][H].y, v.hi[0][H].z, v.hi[0][H].w};
            const unsigned int r1[4] = {v.hi[1][H].x, v.hi[1][H].y, v.hi[1][H].z, v.hi[1][H].w};
            const unsigned int r2[4] = {v.hi[2][H].x, v.hi[2][H].y, v.hi[2][H].z, v.hi[2][H].w};
            const unsigned int r3[4] = {v.hi[3][H].x, v.hi[3][H].y, v.hi[3][H].z, v.hi[3][H].w};
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                const int d = w >> 1;
                const uint2 vb = (w & 1) ? make_uint2(hi_pair(r0[d], r1[d]), hi_pair(r2[d], r3[d]))
                                         : make_uint2(lo_pair(r0[d], r1[d]), lo_pair(r2[d], r3[d]));
                f32x4_t zc = Z[H * 8 + w];
                zc = mfma_k16_16x16x16(pa, vb, zc);
                if constexpr (XLO != 0) {
                    // channel pair d of key e: a dword of the key16 lo row, or two bytes of the e4m3 row converted here (one v_cvt per pair and key)
                    auto lo_pair_of = [&](int e) -> unsigned int {
                        if constexpr (XLO == 2) {
                            const unsigned int b = v.lo[e][H][d >> 1];
                            return (d & 1) ? lo8_pair<1>(b) : lo8_pair<0>(b);
                        } else {
                            return v.lo[e][H][d];
                        }
                    };
                    const unsigned int q0 = lo_pair_of(0), q1 = lo_pair_of(1), q2 = lo_pair_of(2), q3 = lo_pair_of(3);
                    const uint2 vl = (w & 1) ? make_uint2(hi_pair(q0, q1), hi_pair(q2, q3)) : make_uint2(lo_pair(q0, q1), lo_pair(q2, q3));
                    zc = mfma_k16_16x16x16(pah, vl, zc);
                }
                Z[H * 8 + w] = zc;
                if constexpr (LO8B) { if (w & 1) __builtin_amdgcn_sched_barrier(0); }
            }
        }
        __builtin_amdgcn_wave_barrier();                                             // before the next tile overwrites kt / pl
    }

    // ---- after the last tile: l_run = the row sums over the 16 key lanes (the softmax denominators of the wave's share of the row)
    __device__ __forceinline__ void row_sums() {
        if constexpr (LO8B) {                 // (the same exchanges, addressed from the walk's own lane: __shfl_xor keeps a lane id of its own across the tile loop)
            relane();
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float l = l_run[i];
#pragma unroll
                for (int m = 1; m < 16; m *= 2) l += __int_as_float(__builtin_amdgcn_ds_bpermute((lane ^ m) << 2, __float_as_int(l)));
                l_run[i] = l;
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float l = l_run[i];
            l += __shfl_xor(l, 1, 64);
            l += __shfl_xor(l, 2, 64);
            l += __shfl_xor(l, 4, 64);
            l += __shfl_xor(l, 8, 64);
            l_run[i] = l;
        }
    }
    // the wave's un-normalised z -> szw [head][256] fp32 (LDS; may be the wave's own key tile).  hi rows (lanes 0-31) + lo rows (lanes 32-63) of
    // z with ONE half-wave exchange per register pair (v_permlane32_swap): afterwards lanes g < 2 hold the sums of column tiles w = 0..3 and
    // lanes g >= 2 those of w = 4..7 (for head 4 (g & 1) + i), so that every lane stores one float4 per (half, row)
    __device__ __forceinline__ void store_z(float* szw) const {
#pragma unroll
        for (int H = 0; H < 2; ++H)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v[4];
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(Z[H * 8 + w][i]), __float_as_uint(Z[H * 8 + w + 4][i]), false, false);
                    v[w] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
                }
                float* dst = szw + (4 * (g & 1) + i) * C + 128 * H + 8 * n + 4 * (g >> 1);
                *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            }
    }
};

}  // namespace
