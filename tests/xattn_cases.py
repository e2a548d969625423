"""Cases and plain torch references for the cross-attention kernels with hi + lo key / value rows (csrc/xattn_walk.h, xattn_tile.hip,
xattn_fused.hip, xattn_group.hip).  No tests here: tests/test_xattn_cases_cpu.py shows on the CPU that the cases tell a correct fp32-class
kernel from one with a defect in its lo terms, tests/test_gpu_xattn_lo.py holds the kernels to them.

The shared-hi case.  A key row is x = h + l: h is an fp16 number (11-bit significand m * 2^(e-10), m in 1025 .. 2047, random sign per channel)
SHARED by all keys of a query's row, l a per-key remainder with 0.05 <= |l| 2^(10-e) <= 0.45, below half an fp16 ulp of h.  The key16 split of
x therefore gives hi == h bit for bit and lo carries everything that tells the keys of a row apart: without the lo terms every key of a row has
the same logit and z == h_v; with them the logits spread by delta = Qt . l_k and z - h_v = sum_j p_j l_v[j] depends on both lo arrays.  The
queries are scaled per (row, head) so that the standard deviation of delta over the keys of the row is 1.8 (a query whose short row would need
one head scaled more than twice beyond the expected spread is drawn again).  The common logit term Qt . h is
1e4 .. 3e4, so the fp32 rounding of the logits, not the 16-bit formats, sets the floor of a correct kernel (1e-3 .. 1e-2 of max|z - h_v|).

Row lengths sit on the edges of the 16-key tile and on 16 waves +- 1 for 1, 2, 4 and 8 waves (ROW_LENGTHS), in an order that mixes short and
long rows in every block of 8 queries; one row lists every third key of its block (col_idx not contiguous), two rows list the same block.
In every row with two or more keys the key whose logit deviates most from the row's mean is listed LAST, so that a defect that touches only
the ragged last tile shows at the full scale of the row (the second of the two rows that share a block takes what the first one got)."""
import types

import numpy as np
import torch

C, HEADS = 256, 8
TILE = 16
ROW_LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 257, 613)
STRIDE, STRIDED_KEYS, SHARED_KEYS, PAD_KEYS = 3, 40, 37, 5
DELTA_STD = 1.8
LO8_SCALE = 4096.0


def _layout(seed):
    """(row_ptr, col_idx, block_of_key [S], block_of_row [R], sharp_free [R]): rows in launch order, key blocks laid out in a shuffled order."""
    asc = sorted(ROW_LENGTHS)
    seq = []
    for b, extra in enumerate((('strided', STRIDED_KEYS), ('shared', SHARED_KEYS), ('shared', SHARED_KEYS))):
        mine = [('own', n) for n in asc[b::3]]         # every block of 8 queries: a third of the lengths, short to long ...
        blk = []
        while mine:                                    # ... as longest, shortest, second longest, ...: never sorted by length
            blk.append(mine.pop())
            if mine:
                blk.append(mine.pop(0))
        blk.insert(4, extra)
        seq += blk
    g = np.random.Generator(np.random.PCG64(seed))
    blocks, first_shared = [], None                    # (size of the key block) per block; a row -> its block
    block_of_row = []
    for kind, n in seq:
        if kind == 'shared' and first_shared is not None:
            block_of_row.append(first_shared)
            continue
        if kind == 'shared':
            first_shared = len(blocks)
        block_of_row.append(len(blocks))
        blocks.append(n * STRIDE if kind == 'strided' else n)
    start = np.zeros(len(blocks), dtype=np.int64)
    off = PAD_KEYS                                     # a few keys in front that no row lists
    for b in g.permutation(len(blocks)):
        start[b] = off
        off += blocks[b]
    S = off + PAD_KEYS
    block_of_key = np.full(S, len(blocks), dtype=np.int64)          # the padding keys form a block of their own
    for b, n in enumerate(blocks):
        block_of_key[start[b]:start[b] + n] = b
    row_ptr, col = [0], []
    for (kind, n), b in zip(seq, block_of_row):
        col += list(range(start[b], start[b] + blocks[b], STRIDE if kind == 'strided' else 1))
        row_ptr.append(len(col))
    sharp_free = [not (kind == 'shared' and i != seq.index(('shared', SHARED_KEYS))) for i, (kind, n) in enumerate(seq)]
    return (torch.tensor(row_ptr, dtype=torch.int32), torch.tensor(col, dtype=torch.int32), torch.from_numpy(block_of_key),
            torch.tensor(block_of_row), sharp_free)


STRIDED_ROW, SHARED_ROWS = 4, (12, 20)


def _randn(g, shape, scale=1.0):
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def _finish(case):
    case.R, case.S = case.q.shape[0], case.xk32.shape[0]
    case.nk = (case.row_ptr[1:] - case.row_ptr[:-1]).long()
    case.nnz = int(case.col_idx.numel())
    case.pair_row = torch.repeat_interleave(torch.arange(case.R), case.nk)
    case.pair_pos = torch.arange(case.nnz) - case.row_ptr[:-1].long()[case.pair_row]         # position of a pair in its row
    return case


def qk_map(q, Wk):
    """The query map in fp64: Qt[r][h][c] = sum_d q[r][32 h + d] Wk[32 h + d][c]"""
    return torch.einsum('rhd,hdc->rhc', q.double().view(-1, HEADS, 32), Wk.double().view(HEADS, 32, C))


def shared_hi_case(e, seed):
    row_ptr, col, block_of_key, block_of_row, sharp_free = _layout(seed)
    g = np.random.Generator(np.random.PCG64(seed + 1))
    S, R, nb = block_of_key.numel(), block_of_row.numel(), int(block_of_key.max()) + 1
    ulp = 2.0 ** (e - 10)

    def shared(n):
        return torch.from_numpy(g.integers(1025, 2048, (n, C)) * g.choice([-1.0, 1.0], (n, C)) * ulp)

    def remainder():
        return torch.from_numpy(g.uniform(0.05, 0.45, (S, C)) * g.choice([-1.0, 1.0], (S, C)) * ulp)

    hk, hv, lk, lv = shared(nb), shared(nb), remainder(), remainder()
    Wk, Wv, bv = _randn(g, (C, C), 0.06), _randn(g, (C, C), 0.06), _randn(g, (C,))
    q = torch.zeros((R, C), dtype=torch.float64)
    rp, cl = row_ptr.tolist(), col.long()
    rms = float(lk.pow(2).mean().sqrt())
    for r in range(R):
        cols = cl[rp[r]:rp[r + 1]]
        for _ in range(10000):
            # the spread of a short row is a matter of chance (two keys: |delta_1 - delta_2| / 2); a query that would need one head scaled far beyond
            # the others (a common term beyond the 1e4 .. 3e4 of the other rows, and an fp32 floor to match) is drawn again
            q[r] = _randn(g, (C,), 0.3).double()
            qk = qk_map(q[r:r + 1], Wk)[0]
            expected = qk.norm(dim=1) * rms            # of remainders of this distribution
            std = (lk[cols] @ qk.T).std(0, unbiased=False) if len(cols) >= 2 else expected
            if bool(((std >= 0.5 * expected) & (std <= 2.0 * expected)).all()):
                break
        else:
            raise RuntimeError('shared_hi_case: no query with an even spread; another seed')
        q[r] = (q[r].view(HEADS, 32) * (DELTA_STD / std)[:, None]).view(C)
    q = q.float()
    qk = qk_map(q, Wk)
    for r in range(R):                                 # the sharpest key of a row goes last
        cols = cl[rp[r]:rp[r + 1]]
        if len(cols) >= 2 and sharp_free[r]:
            d = lk[cols] @ qk[r].T                     # [nk, 8]
            j = int((d - d.mean(0)).abs().max(1).values.argmax())
            a, b = int(cols[j]), int(cols[-1])
            lk[[a, b]] = lk[[b, a]]
    case = types.SimpleNamespace(kind='shared_hi', e=e, row_ptr=row_ptr, col_idx=col, q=q, Wk=Wk, Wv=Wv, bv=bv,
                                 xk32=(hk[block_of_key] + lk).float(), xv32=(hv[block_of_key] + lv).float(),
                                 hk=hk[block_of_row].float(), hv=hv[block_of_row].float())
    return _finish(case)


def random_case(seed):
    """The CSR of the shared-hi case on asymmetric unit-variance rows, queries of 0.3, one of them (a 129-key row) eight times as sharp:
    the operands of tests/test_gpu_kernels.py::test_xattn_tile_equals_projected_attention."""
    row_ptr, col, block_of_key, block_of_row, _ = _layout(seed)
    g = np.random.Generator(np.random.PCG64(seed + 2))
    S, R = block_of_key.numel(), block_of_row.numel()
    q = _randn(g, (R, C), 0.3)
    nk = (row_ptr[1:] - row_ptr[:-1]).tolist()
    q[nk.index(129)] *= 8.0
    case = types.SimpleNamespace(kind='random', e=None, row_ptr=row_ptr, col_idx=col, q=q, xk32=_randn(g, (S, C)), xv32=_randn(g, (S, C)),
                                 Wk=_randn(g, (C, C), 0.06), Wv=_randn(g, (C, C), 0.06), bv=_randn(g, (C,)), hk=None, hv=None)
    return _finish(case)


# ------------------------------------------------------------------------------------------------ the formats, restated in torch
def split_key16(x):
    """fp32 -> (hi, lo) fp16 with x ~ hi + lo: csrc/common.h split_k16x2 (inside the fp16 range)"""
    hi = x.to(torch.float16)
    return hi, (x - hi.float()).to(torch.float16)


def lo8_encode(lo):
    """key16 lo rows -> e4m3 "lo8" bytes: round-to-nearest-even of lo * 2^12, clamped to +-448 (csrc/common.h lo8_pack4)"""
    return (lo.float() * LO8_SCALE).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def lo8_decode(b, scale=LO8_SCALE):
    return (b.view(torch.float8_e4m3fn).float() / scale).to(torch.float16)


def qt_emulated(case):
    """[R,8,256] fp64: the hi + lo pair that the query map stores, from its fp64 statement (the CPU stand-in for _unpack_qt of ops.xattn_qmap)"""
    hi, lo = split_key16(qk_map(case.q, case.Wk).float())
    return hi.double() + lo.double()


# ------------------------------------------------------------------------------------------------ the references
def attend(case, Qt, khi, klo, vhi, vlo, dtype=torch.float64, keep_k=None, keep_v=None):
    """Masked attention of the case on the DECODED operands k = khi + klo, v = vhi + vlo ([S,256]; klo / vlo may be None), Qt [R,8,256], all
    converted to `dtype` first (fp64: the reference; fp32: a plain fp32 evaluation, the yardstick).  keep_k / keep_v [nnz] bool: the lo half of a
    (query, key) pair is dropped where False (the emulated defects).  Returns logits [8,nnz] in CSR order, z [R,8,256], ctx [R,256] = Wv_h z_h + bv;
    a row without a key has z = 0 and ctx = bv and is excluded by row_errors."""
    Qt = Qt.to(dtype)
    rp, col = case.row_ptr.tolist(), case.col_idx.long()
    logits, z = torch.zeros((HEADS, case.nnz), dtype=dtype), torch.zeros((case.R, HEADS, C), dtype=dtype)

    def rows(hi, lo, cols, keep, a, b):
        x = hi[cols].to(dtype)
        if lo is not None:
            l = lo[cols].to(dtype)
            x = x + (l if keep is None else l * keep[a:b, None].to(dtype))
        return x

    for r in range(case.R):
        a, b = rp[r], rp[r + 1]
        if b > a:
            lg = Qt[r] @ rows(khi, klo, col[a:b], keep_k, a, b).T
            logits[:, a:b] = lg
            z[r] = torch.softmax(lg, -1) @ rows(vhi, vlo, col[a:b], keep_v, a, b)
    ctx = torch.einsum('hdc,rhc->rhd', case.Wv.to(dtype).view(HEADS, 32, C), z).reshape(case.R, C) + case.bv.to(dtype)
    return types.SimpleNamespace(logits=logits, z=z, ctx=ctx)


def bases(case, lo_free):
    """What the lo halves move the results away from: (z base [R,1,256], ctx base [R,256]) = (h_v, Wv h_v + bv) for the shared-hi case with lo rows,
    0 otherwise (the random case; hi-only rows, where the result itself is the scale)."""
    if case.kind != 'shared_hi' or lo_free:
        return 0.0, 0.0
    hv = case.hv.double()
    return hv[:, None, :], (hv @ case.Wv.double().T) + case.bv.double()


def row_errors(got, want, base=0.0):
    """[R] fp64: per row max|got - want| / max|want - base| over everything behind the first dimension"""
    got, want = got.detach().double().cpu(), want.double()
    R = want.shape[0]
    return (got - want).abs().reshape(R, -1).amax(1) / (want - base).abs().reshape(R, -1).amax(1)


def logit_row_errors(case, got, want, centre):
    """[R] fp64 for logits [8,nnz] in CSR order: per row max|got - want| / max|want|; centre: both as deviations from their mean over the keys of
    the row, per head (the shared-hi case: the common term of 1e4 cancels in the softmax).  NaN for rows without a key, and, centred, for one key."""
    got, want = got.detach().double().cpu(), want.double()
    rp = case.row_ptr.tolist()
    out = torch.full((case.R,), float('nan'), dtype=torch.float64)
    for r in range(case.R):
        a, b = rp[r], rp[r + 1]
        if b - a >= (2 if centre else 1):
            g_, w_ = got[:, a:b], want[:, a:b]
            if centre:
                g_, w_ = g_ - g_.mean(1, keepdim=True), w_ - w_.mean(1, keepdim=True)
            out[r] = (g_ - w_).abs().max() / w_.abs().max()
    return out
