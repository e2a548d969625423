// Cross attention of a decoder layer in ONE launch (round 5): query map -> tile attention -> context map, fused per block of 8 or 12 queries.
//
// Replaces the three launches of csrc/xattn_tile.hip (xattn_qmap_kernel, xattn_tile_kernel, xattn_ctxmap_kernel) for
// PETRMultiheadAttention's core (MU/petr_transformer.py:426-513) on rows of similar length (the S path: a query reads the 49 cells of its own
// RoI and of the few RoIs matched to it).  The arithmetic is the same, operation for operation (raw key space, see xattn_tile.hip: the K / V
// in_proj ride on the query side, the key side reads the unprojected key16 hi + lo rows), so the results are BITWISE those of the three
// kernels with one wave per query (tests/test_gpu_kernels.py::test_xattn_fused_equals_the_three_kernels); what disappears are the two
// intermediates of that decomposition -- Qt (8 KB per query: the mapped query as a 16 x 256 key16 MFMA operand) and z (8 KB: the per-head
// context sums in the key space) -- which the three kernels write to and read back from HBM: 16 of the ~121 KB a query of the index-exact
// route moves per layer, and two launches of six.
//
// Block = 8 queries, 8 waves (two per SIMD), LDS 132 KB:
//   phase A  wave = head h: Qt_h of the 8 queries (split-precision MFMAs on the fp32 query, packed weights WA from L2) -> LDS [query][head][1 KB]
//   phase B  wave = query w: its Qt operand into 32 registers, then the tile walk of xattn_tile_kernel<1, false, XLO> over its CSR row (xattn_walk.h) (key
//            tiles of 16 rows through the wave's 16 KB of LDS (12 KB in blocks of 12) -- which alias the Qt area once every wave holds its operand); the un-normalised
//            context sums z and the softmax denominators go to LDS
//   phase C  wave = head h: ctx[:, 32 h .. 32 h + 31] = Wv_h z_h / l_h + bv for the 8 queries (packed weights WB from L2), NaN / 0 for a row
//            without a key, written to HBM as the [R, 256] fp32 rows the out-projection kernel reads.
// A block streams the packed weights of both maps (512 KB of hi + lo fragments) from L2 once per block = 64 KB per query in blocks of 8 against the
// ~105 KB of key / value rows it gathers from HBM; the blocks of a launch are out of phase after the first round, so the map phases of one
// CU overlap the gathers of the others.
// Block = 12 queries, 12 waves (three per SIMD: 168 registers per lane, none in scratch), LDS 151 KB -- batch-sized launches with e4m3 lo rows: the lo key
// tile stays 4 KB of bytes in LDS and is widened at the fragment read (12 KB per query instead of 16), the map phases request a head's weights in two halves,
// the waves beyond the 8 heads only gather.  A block's time hardly depends on its query count (two fixed map phases + the walk of ONE query per wave), and the
// map MFMAs compute 16 query columns whatever QB is: 4800 queries are 400 blocks instead of 600, two rounds of CUs instead of three, 43 KB of map weights per
// query instead of 64.  Same arithmetic per query in the same order: bitwise the 8-query instance (tests/test_gpu_xattn_fused_qb.py).  Measured
// (profiles/xattn_qb_kernel_stats.txt): 106.8 -> 95.5 us per 16-sample cfg2_s launch.  Not built: 16 queries per block for rows without lo halves (8 KB
// per tile), by the same reasoning.  Rows of very different length (the T path: 1 .. 400 keys) would wait for the longest of the block at
// the barrier between B and C: the engine keeps the three kernels there.
// Round 6 experiments that lost and are gone from the source (profiles/r06_xattn_fused_lo8_experiments.txt; LOG.md): the key rows of tile t + 1
// requested in front of tile t's arithmetic (slower: 1).  The tile loops alone, without the map phases, as a timing experiment (3).  The
// weight fragments of phase A in three batches between the MFMA groups (slower: 6).  MODE.FP16_OVFL for the whole kernel (7: faster by 2 %, but
// a NaN in a key row, a value row or the query no longer reached the output, and a poisoned input frame must stay visible).
#include "xattn_walk.h"
#include <stdlib.h>
#ifndef MV2D_XF_QB_DEFAULT
#define MV2D_XF_QB_DEFAULT 8
#endif
#ifndef MV2D_XF_QB_BATCH
#define MV2D_XF_QB_BATCH 12                                   // batch-sized launches with e4m3 lo rows
#endif
// How the queries of a batch-sized launch (more blocks of QB than one round of CUs) are dealt to blocks:
//   XF_DEAL_ROUNDS  the block count rounded up to whole rounds of CUs while a block keeps >= QB / 2 queries (4800 queries: 768 blocks of 6-7)
//   XF_DEAL_FULL    ceil(R / QB) blocks of QB queries (600 blocks of 8): the fewest blocks, i.e. the fewest map phases and the least CU-time
// The default is XF_DEAL_FULL: the library sizes batch launches for SEVERAL launch sequences in flight.  A block holds a whole CU (132 KB of LDS) and
// pays both map phases whatever its query count, so what a launch costs the other streams is blocks x time per block.  Measured on an MI355X
// (profiles/batch_shapes_kernel_stats.txt; 16 cfg2_s samples per launch, R = 4800): the launch takes 104.8 us either way in the four-stream loop and
// 105.8 / 105.2 us alone on an idle GPU, on 768 / 600 CU slots; four streams complete 10524 -> 10720 samples/s (+1.9 %), one stream is unchanged
// (6752 -> 6750).  MV2D_XF_DEAL=1 restores whole rounds.  The policy is a function of the row count only: neither a sample's result nor a graph's
// shape depends on what else runs.
enum { XF_DEAL_ROUNDS = 1, XF_DEAL_FULL = 2 };
#ifndef MV2D_XF_DEAL_DEFAULT
#define MV2D_XF_DEAL_DEFAULT XF_DEAL_FULL
#endif
constexpr int XF_DEAL_DEFAULT = MV2D_XF_DEAL_DEFAULT;

#ifdef MV2D_XF_TRACE
__device__ long long g_xf_trace[32];
#define XF_STAMP(i) do { if (blockIdx.x == MV2D_XF_TRACE && threadIdx.x == 0) g_xf_trace[i] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#else
#define XF_STAMP(i) do {} while (0)
#endif

namespace {

// per wave: key tile hi (8 KB) | key tile lo (8 KB of key16; above 8 queries per block 4 KB of e4m3 bytes: XattnWalk's LO8B); phase A / C: Qt / z of query `wave`
// in the first 8 KB.  (The byte tile under blocks of 8 measured 108.9 against 106.8 us per launch: it stays with the instance that needs it.)
template <int XLO, int QB> constexpr bool XF_SLIM = XLO == 2 && QB > 8;
template <int XLO, int QB> constexpr int WAVE_LDS = XF_SLIM<XLO, QB> ? 12288 : 16384;

// QB = 8: one block per CU (132 KB of LDS); QB = 4 (round 6): 66 KB, two blocks per CU -- the map phases of one block (packed weights from L2, the
// gather idle) run under the tile loop of the other; a wave then maps two heads in phases A and C
// XLO: 0 = key16 rows alone, 1 = hi + key16 lo rows, 2 = hi + e4m3 lo rows (common.h "lo8"; see xattn_tile_kernel)
template <int XLO, int QB>
__device__ __forceinline__ int xf_slot(int n) {                 // a valid query slot for each of the 16 operand columns / rows of a map MFMA
    if constexpr ((QB & (QB - 1)) == 0) return n & (QB - 1);
    else return n < QB ? n : 0;
}

template <int XLO, int QB>
__global__ __launch_bounds__(64 * QB, 2) void xattn_fused_kernel(const float* __restrict__ q, const uint4* __restrict__ WA_hi, const uint4* __restrict__ WA_lo,
                                                                const uint4* __restrict__ WB_hi, const uint4* __restrict__ WB_lo, const float* __restrict__ bv,
                                                                const unsigned short* __restrict__ Xk, const unsigned short* __restrict__ Xv,
                                                                const unsigned short* __restrict__ Xk_lo, const unsigned short* __restrict__ Xv_lo,
                                                                const int* __restrict__ row_ptr, const int* __restrict__ col_idx, float* __restrict__ ctx,
                                                                int R, int empty_nan, const int* __restrict__ order, int nblk) {
    constexpr int SMEM = QB * WAVE_LDS<XLO, QB> + QB * 512 + QB * HEADS * 4 + 3 * QB * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];
    // (SLIM, the 12-query instance: wave and everything derived from it -- the CSR row ends, the LDS areas -- as scalars, and the hardware's lane id, which is
    //  the one the shuffles use: registers are what caps the queries per block.  The other instances are instruction for instruction what they were.)
    constexpr bool SLIM = XF_SLIM<XLO, QB>;
    const int tid = threadIdx.x, lane = SLIM ? (int)__lane_id() : tid & 63, wave = SLIM ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
    const int n = lane & 15, g = lane >> 4;
    float* lsum = reinterpret_cast<float*>(smem + QB * WAVE_LDS<XLO, QB> + QB * 512);         // [query][head] softmax denominators
    int* rq = reinterpret_cast<int*>(smem + QB * WAVE_LDS<XLO, QB> + QB * 512 + QB * HEADS * 4);       // [query slot] -> query row, then the ends of its CSR row
    int* rbeg = rq + QB;
    int* rend = rq + 2 * QB;
    // XCD-chunked block order (block b runs on XCD b % 8): every XCD works through one contiguous range of query slots; optional launch order
    // of the queries (the S path ranks them by the smallest RoI they list, so that matched RoIs share an L2).  Speed only.
    // The R query slots are dealt EVENLY to nblk >= ceil(R / QB) blocks; the host chooses nblk (XF_DEAL_* above: ceil(R / QB) for a batch-sized launch,
    // up to one block per CU for a small one).  Rounding 600 blocks of 8 up to 768 of 6-7 -- three whole rounds of one block per CU -- was measured at
    // 140 -> 112 us per layer when that rule was written; on today's kernel both shapes take 105 us (profiles/batch_shapes_kernel_stats.txt), and the
    // 600 leave 168 CU slots per launch to the other streams.
    const int blk = xcd_chunked(blockIdx.x, nblk);
    const int slot0 = (int)((long long)blk * R / nblk), nq = (int)((long long)(blk + 1) * R / nblk) - slot0;
    if (nq <= 0) return;
    XF_STAMP(0);
    if (tid < QB) {
        const int s = slot0 + min(tid, nq - 1);
        const int r_ = order ? order[s] : s;
        rq[tid] = r_;
        rbeg[tid] = row_ptr[r_];
        rend[tid] = row_ptr[r_ + 1];
    }
    __syncthreads();
    XF_STAMP(1);
    // Round 6 (per-phase stamps, tools/xf_trace.py: 43 % of a block's time was the wait for a tile's key rows, the first tile's behind three dependent round
    // trips -- row ends, key indices, rows -- that only started after phase A): the wave's CSR row ends come with the slot table, the indices of its first
    // tile are requested in front of phase A and the hi + lo key rows of that tile in the middle of it, so that they travel under the query maps.
    const int beg = SLIM ? __builtin_amdgcn_readfirstlane(rbeg[wave]) : rbeg[wave], end = SLIM ? __builtin_amdgcn_readfirstlane(rend[wave]) : rend[wave];
    const int ntile = wave < nq ? (end - beg + 15) >> 4 : 0;          // (waves beyond the block's queries: no tiles; their z / l are never read)
    int idx_next = ntile > 0 ? col_idx[min(beg + n, end - 1)] : 0;
    // (a wave's Qt operand lies in its OWN area of WAVE_LDS, which only the wave itself overwrites with key tiles in phase B: no barrier needed there)
    typedef XattnWalk<XLO, false, XF_SLIM<XLO, QB>> Walk;
    Walk walk(Xk, Xv, Xk_lo, Xv_lo, lane, beg, end, reinterpret_cast<uint4*>(smem + wave * WAVE_LDS<XLO, QB>), reinterpret_cast<uint4*>(smem + wave * WAVE_LDS<XLO, QB>) + 512,
           reinterpret_cast<float*>(smem + QB * WAVE_LDS<XLO, QB>) + wave * 128);
    typename Walk::KRows k0;
    // More than 8 queries per block: three waves share a SIMD, i.e. 168 registers per lane.  The map phases then request a head's weight fragments in
    // NP = 2 halves (64 registers next to the 48 of the first tile's key rows, not 128), one L2 round trip more per phase; every output element keeps
    // its own accumulator and its three MFMAs in the order of NP = 1.  The waves beyond the 8 heads map nothing and request their key rows at once.
    constexpr int NP = QB > 8 ? 2 : 1, TP = 16 / NP, UP = 8 / NP;
    if (QB > HEADS && wave >= HEADS && ntile > 0) walk.request_k(idx_next, k0);
    // ---------------------------------------------------------------- phase A: query maps, wave = head
    for (int h = wave; h < HEADS; h += QB) {
        const int r = rq[xf_slot<XLO, QB>(n)];
        const float* qp = q + (long long)r * C + 32 * h + 8 * g;
        // (the query values are REQUESTED here and split behind the weight requests: split first, hipcc waited for them -- a full round trip -- before it issued
        //  the first weight load: 3.4 k of a block's 62 k cycles, round 6 stamps)
        const float4 q0 = *reinterpret_cast<const float4*>(qp), q1 = *reinterpret_cast<const float4*>(qp + 4);
        const uint4* wh = WA_hi + (long long)h * 16 * 64 + lane;
        const uint4* wl = WA_lo + (long long)h * 16 * 64 + lane;
        uint4* qt = reinterpret_cast<uint4*>(smem + xf_slot<XLO, QB>(n) * WAVE_LDS<XLO, QB>) + h * 64;      // this lane's query, this head: 64 chunks of 16 B
        // ALL 32 weight fragments of the head are requested before the first MFMA (128 registers, free in this phase): the first build left the
        // loads next to their MFMAs and the ISA showed 24 serialised L2 round trips per block and phase (tools/isa_waits.sh)
        Frag bh, bl;
#pragma unroll
        for (int part = 0; part < NP; ++part) {
            u32x4 wa_h[TP], wa_l[TP];
#pragma unroll
            for (int t = 0; t < TP; ++t) {
                wa_h[t] = *reinterpret_cast<const u32x4*>(wh + (part * TP + t) * 64);
                wa_l[t] = *reinterpret_cast<const u32x4*>(wl + (part * TP + t) * 64);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (part == 0) {
                XF_STAMP(20);
                split8(q0, q1, bh, bl);
            }
#pragma unroll
            for (int uu = 0; uu < UP; ++uu) {
                const int u = part * UP + uu;
                if (u == 1) XF_STAMP(21);
                if (u == 4) XF_STAMP(22);
                f32x4_t a[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    f32x4_t c = {0.f, 0.f, 0.f, 0.f};
                    c = mfma_q16_16x16x32(wa_l[2 * uu + k], bh.v, c);
                    c = mfma_q16_16x16x32(wa_h[2 * uu + k], bl.v, c);
                    c = mfma_q16_16x16x32(wa_h[2 * uu + k], bh.v, c);
                    a[k] = c;
                }
                Frag hi, lo;
                split8_k16(make_float4(a[0][0], a[0][1], a[0][2], a[0][3]), make_float4(a[1][0], a[1][1], a[1][2], a[1][3]), hi, lo);
                if (n < QB) {
                    qt[u * 8 + g * 2] = hi.u;
                    qt[u * 8 + g * 2 + 1] = lo.u;
                }
                // (all weight fragments of the head have been requested: the rows queue behind them; late enough for their 64 registers)
                if (u == (XLO ? 5 : 3) && h == wave && ntile > 0) walk.request_k(idx_next, k0);
            }
            if (NP > 1) __builtin_amdgcn_sched_barrier(0);      // (the next half's requests stay behind this half's MFMAs: its registers are these)
        }
    }
    XF_STAMP(23);
    // (LDS only: __syncthreads() would also wait for the key rows that are still in flight -- vmcnt(0) -- and put their latency back in front of phase B)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    XF_STAMP(2);
    // ---------------------------------------------------------------- phase B: tile attention, wave = query
    // (SLIM: from here on the lane's coordinates are the walk's copy, so that one value lives across the tile loop)
    {
        const int nb = SLIM ? walk.n : n, gb = SLIM ? walk.g : g;
        const uint4* qp = reinterpret_cast<const uint4*>(smem + wave * WAVE_LDS<XLO, QB>) + (nb & 7) * 64 + gb * 2 + (nb >> 3);
#pragma unroll
        for (int s = 0; s < 8; ++s) walk.qa[s].u = qp[s * 8];
    }
    walk.reset();
    // the first tile's key rows were requested during phase A: into LDS right away (the wave's Qt operand sits in qa by now)
    if (ntile > 0) walk.stage_k(k0);
#pragma nounroll      // (nor peeled: tile 0 differs only in its key gather; hipcc otherwise emits the hi-only tile arithmetic twice)
    for (int tt = 0; tt < ntile; ++tt) {
        const int myidx = idx_next;
        if (tt + 1 < ntile) idx_next = col_idx[min(beg + 16 * (tt + 1) + (SLIM ? walk.n : n), end - 1)];
        typename Walk::VRows v;
        walk.gather(myidx, tt > 0, v);
        XF_STAMP(3 + 2 * min(tt, 5));
        walk.compute(tt, v, myidx);
        XF_STAMP(4 + 2 * min(tt, 5));
    }
    // ---- denominators (row sums over the 16 key lanes) and the un-normalised z of the query into the wave's own LDS area ([head][256] fp32 = 8 KB)
    walk.row_sums();
    {
        const int nb = SLIM ? walk.n : n, gb = SLIM ? walk.g : g;
        if (nb == 0 && gb < 2) {
#pragma unroll
            for (int i = 0; i < 4; ++i) lsum[wave * HEADS + 4 * gb + i] = walk.l_run[i];
        }
    }
    walk.store_z(reinterpret_cast<float*>(smem + wave * WAVE_LDS<XLO, QB>));
    XF_STAMP(15);
    __syncthreads();
    XF_STAMP(16);
    // ---------------------------------------------------------------- phase C: context maps, wave = head
    // (SLIM: the lane's coordinates derived again, opaquely: what phase C computes from them would otherwise be held in registers across the tile loop)
    const int lc = SLIM ? Walk::fresh(walk.lane) : lane, nc = SLIM ? lc & 15 : n, gc = SLIM ? lc >> 4 : g;
    for (int h = wave; h < HEADS; h += QB) {
        const int j = xf_slot<XLO, QB>(nc);
        const float* zp = reinterpret_cast<const float*>(smem + j * WAVE_LDS<XLO, QB>) + h * C + 8 * gc;
        // (xattn_tile_kernel normalises when it merges its waves: num * rcp(den), the factor of the single wave being exp2(0) = 1)
        const float rl = __builtin_amdgcn_rcpf(lsum[j * HEADS + h]);
        const uint4* wh = WB_hi + (long long)h * 16 * 64 + lc;
        const uint4* wl = WB_lo + (long long)h * 16 * 64 + lc;
        f32x4_t acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        int rr_[4], rp0_[4], rp1_[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rr_[i] = rq[xf_slot<XLO, QB>(4 * gc + i)];
            rp0_[i] = rbeg[xf_slot<XLO, QB>(4 * gc + i)];
            rp1_[i] = rend[xf_slot<XLO, QB>(4 * gc + i)];
        }
        const float bv0 = bv[32 * h + nc], bv1 = bv[32 * h + 16 + nc];
#pragma unroll
        for (int part = 0; part < NP; ++part) {
            u32x4 wb_h[TP], wb_l[TP];                      // (all fragments of the head, or of this half, first, like phase A; and what the epilogue reads)
#pragma unroll
            for (int t = 0; t < TP; ++t) {
                wb_h[t] = *reinterpret_cast<const u32x4*>(wh + (part * TP + t) * 64);
                wb_l[t] = *reinterpret_cast<const u32x4*>(wl + (part * TP + t) * 64);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ss = 0; ss < UP; ++ss) {
                const int s = part * UP + ss;
                float4 x0 = *reinterpret_cast<const float4*>(zp + 32 * s);
                float4 x1 = *reinterpret_cast<const float4*>(zp + 32 * s + 4);
                x0 = make_float4(x0.x * rl, x0.y * rl, x0.z * rl, x0.w * rl);
                x1 = make_float4(x1.x * rl, x1.y * rl, x1.z * rl, x1.w * rl);
                Frag ah, al;
                split8(x0, x1, ah, al);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    acc[nt] = mfma_q16_16x16x32(al.v, wb_h[ss * 2 + nt], acc[nt]);
                    acc[nt] = mfma_q16_16x16x32(ah.v, wb_l[ss * 2 + nt], acc[nt]);
                    acc[nt] = mfma_q16_16x16x32(ah.v, wb_h[ss * 2 + nt], acc[nt]);
                }
            }
            if (NP > 1) __builtin_amdgcn_sched_barrier(0);
        }
        if (4 * gc < QB) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int js = 4 * gc + i;
                if (js < nq) {
                    const int rr = rr_[i];
                    const bool empty = rp1_[i] <= rp0_[i];
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const int col = 32 * h + 16 * nt + nc;
                        float v = acc[nt][i] + (nt ? bv1 : bv0);
                        if (empty) v = empty_nan ? __uint_as_float(0x7fc00000u) : 0.f;
                        ctx[(long long)rr * C + col] = v;
                    }
                }
            }
        }
    }
    XF_STAMP(17);
}

}  // namespace

#ifdef MV2D_XF_TRACE
extern "C" int mv2d_xf_trace_read(long long* host, int n) { return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_xf_trace), n * sizeof(long long)) == hipSuccess ? 0 : -2; }
#endif

// C-ABI: include/mv2d_hip.h
// deal: the block count of a batch-sized launch (more blocks than one round of CUs) as a launch policy -- 0 = the library's default,
// 1 = whole rounds (XF_DEAL_ROUNDS), 2 = ceil(R / QB) full blocks (XF_DEAL_FULL).  Which block computes a query changes, how it is computed does not.
// qb: the queries per block -- 0 = the library's choice (e4m3 lo rows: MV2D_XF_QB_BATCH for a batch-sized launch, i.e. more than one round of CUs in
// blocks of 8; 8 otherwise), 4 or 8 on every route, 12 with e4m3 lo rows only (12 KB of LDS per query).  A launch policy like deal.
extern "C" int mv2d_xattn_fused_fwd_q(const float* q, const void* WA_hi, const void* WA_lo, const void* WB_hi, const void* WB_lo, const float* bv,
                                      const void* Xk, const void* Xv, const void* Xk_lo, const void* Xv_lo, const int* row_ptr, const int* col_idx,
                                      float* ctx, int R, int empty_nan, const int* order, int lo_fmt, int deal, int qb, void* stream) {
    MV2D_CHECK_ARG(deal >= 0 && deal <= 2, "mv2d_xattn_fused_fwd_q: deal is 0 (default), 1 (whole rounds) or 2 (full blocks)");
    MV2D_CHECK_ARG(qb == 0 || qb == 4 || qb == 8 || (qb == 12 && Xk_lo && lo_fmt == 1), "mv2d_xattn_fused_fwd_q: qb is 0 (default), 4 or 8, or 12 with e4m3 lo rows");
    MV2D_CHECK_ARG(lo_fmt == 0 || (lo_fmt == 1 && Xk_lo), "mv2d_xattn_fused_fwd: lo_fmt is 0 (key16 lo rows) or 1 (e4m3 lo rows; needs the lo rows)");
    MV2D_CHECK_ARG(q && WA_hi && WA_lo && WB_hi && WB_lo && bv && Xk && Xv && row_ptr && col_idx && ctx && R >= 0, "mv2d_xattn_fused_fwd: bad args");
    MV2D_CHECK_ARG((Xk_lo == nullptr) == (Xv_lo == nullptr), "mv2d_xattn_fused_fwd: Xk_lo and Xv_lo come together");
    MV2D_CHECK_ARG(((uintptr_t)q & 15) == 0 && ((uintptr_t)WA_hi & 15) == 0 && ((uintptr_t)WA_lo & 15) == 0 && ((uintptr_t)WB_hi & 15) == 0 &&
                       ((uintptr_t)WB_lo & 15) == 0 && ((uintptr_t)Xk & 15) == 0 && ((uintptr_t)Xv & 15) == 0 && ((uintptr_t)Xk_lo & 15) == 0 &&
                       ((uintptr_t)Xv_lo & 15) == 0, "mv2d_xattn_fused_fwd: operands must be 16-byte aligned");
    if (R == 0) return MV2D_OK;
    static int n_cu = 0;
    if (n_cu == 0) {
        hipDeviceProp_t prop;
        int dev = 0;
        n_cu = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }
    // queries per block: 8 (one block per CU), 4 (two per CU: the map phases of one block under the tile loop of the other), or with e4m3 lo rows 12
    // (one per CU, three waves per SIMD).  MV2D_XF_QB=4 / 8 / 12 forces it for A/B runs (12 on the e4m3 route only); the entry's argument wins.
    // (10 was measured on the launch alone, profiles/xattn_qb_kernel_stats.txt 3, and is not built: like any other value it leaves the default in place.)
    static const int qb_env = [] { const char* e = getenv("MV2D_XF_QB"); return e ? atoi(e) : 0; }();
    const bool lo8 = Xk_lo && lo_fmt == 1;
    int QB = qb ? qb : (qb_env == 4 || qb_env == 8 || (qb_env == 12 && lo8) ? qb_env : 0);
    if (QB == 0) QB = lo8 && (R + MV2D_XF_QB_DEFAULT - 1) / MV2D_XF_QB_DEFAULT > n_cu ? MV2D_XF_QB_BATCH : MV2D_XF_QB_DEFAULT;
    const int slots = n_cu * (QB == 4 ? 2 : 1);               // blocks of a round
    int nblk = (R + QB - 1) / QB;
    if (nblk > slots) {
        // a batch-sized launch: the dealing policy (above XF_DEAL_DEFAULT).  MV2D_XF_DEAL=1 / 2 forces it for A/B runs; the entry's argument wins.
        static const int deal_env = [] { const char* e = getenv("MV2D_XF_DEAL"); return e ? atoi(e) : 0; }();
        const int policy = deal ? deal : (deal_env == XF_DEAL_ROUNDS || deal_env == XF_DEAL_FULL ? deal_env : XF_DEAL_DEFAULT);
        if (policy == XF_DEAL_ROUNDS) {                       // whole rounds, as long as a block keeps >= QB / 2 queries
            const int up = (nblk + slots - 1) / slots * slots;
            if ((long long)up * (QB / 2) <= R) nblk = up;
        }                                                     // XF_DEAL_FULL: ceil(R / QB) blocks, dealt evenly: QB - 1 or QB queries each
    } else {
        // a small launch (one sample: 300 queries = 38 blocks of 8 on a 256-CU chip): spread it, down to two queries per block -- the blocks stream
        // the map weights from L2 either way, and the launch is bound by the longest block (26.5 -> ~14 us per layer at R = 300)
        const int spread = R / 2 < n_cu ? R / 2 : n_cu;
        if (spread > nblk) nblk = spread;
    }
    const dim3 grid(nblk), block(64 * QB);
#define MV2D_XF(XLO_, QB_) hipLaunchKernelGGL((xattn_fused_kernel<XLO_, QB_>), grid, block, 0, (hipStream_t)stream, q, (const uint4*)WA_hi, (const uint4*)WA_lo, \
                                              (const uint4*)WB_hi, (const uint4*)WB_lo, bv, (const unsigned short*)Xk, (const unsigned short*)Xv,                     \
                                              (const unsigned short*)Xk_lo, (const unsigned short*)Xv_lo, row_ptr, col_idx, ctx, R, empty_nan, order, nblk)
    if (lo8) { if (QB == 4) MV2D_XF(2, 4); else if (QB == 12) MV2D_XF(2, 12); else MV2D_XF(2, 8); }
    else if (Xk_lo) { if (QB == 4) MV2D_XF(1, 4); else MV2D_XF(1, 8); }
    else { if (QB == 4) MV2D_XF(0, 4); else MV2D_XF(0, 8); }
#undef MV2D_XF
    MV2D_LAUNCH_CHECK();
    return MV2D_OK;
}

extern "C" int mv2d_xattn_fused_fwd_p(const float* q, const void* WA_hi, const void* WA_lo, const void* WB_hi, const void* WB_lo, const float* bv,
                                      const void* Xk, const void* Xv, const void* Xk_lo, const void* Xv_lo, const int* row_ptr, const int* col_idx,
                                      float* ctx, int R, int empty_nan, const int* order, int lo_fmt, int deal, void* stream) {
    return mv2d_xattn_fused_fwd_q(q, WA_hi, WA_lo, WB_hi, WB_lo, bv, Xk, Xv, Xk_lo, Xv_lo, row_ptr, col_idx, ctx, R, empty_nan, order, lo_fmt, deal, 0, stream);
}

extern "C" int mv2d_xattn_fused_fwd(const float* q, const void* WA_hi, const void* WA_lo, const void* WB_hi, const void* WB_lo, const float* bv,
                                    const void* Xk, const void* Xv, const void* Xk_lo, const void* Xv_lo, const int* row_ptr, const int* col_idx,
                                    float* ctx, int R, int empty_nan, const int* order, int lo_fmt, void* stream) {
    return mv2d_xattn_fused_fwd_p(q, WA_hi, WA_lo, WB_hi, WB_lo, bv, Xk, Xv, Xk_lo, Xv_lo, row_ptr, col_idx, ctx, R, empty_nan, order, lo_fmt, 0, stream);
}
