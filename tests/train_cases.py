"""Cases and plain torch references for the attention and reduction kernels of the TRAINING route: the sparse cross attention
and its backward (csrc/attention.hip: sparse_xattn_kernel<8, 4>, sparse_xattn_bwd_q_kernel<4 | 16>, sparse_xattn_bwd_kv_kernel,
sparse_xattn_bwd_kv_split_kernel), the dense block of the denoising rows (csrc/dense_attn.hip), the self attention with the denoising mask
(self_attn_kernel<true>, and csrc/self_attn_x3.hip with the mask), and the row reductions of csrc/train_ops.hip (ln_bwd_kernel, colsum_kernel,
softmax_bwd_rows_kernel).  No tests here: tests/test_train_cases_cpu.py shows on the CPU what the cases can carry, tests/test_gpu_train_edges.py
holds the kernels to them.  Needs neither the library nor a GPU.

Every reference is a function of dtype: float64 is the reference, float32 the plain torch evaluation of the same formulas.  The ROW ERROR of an
output is, per row, max|got - want| / max(max|want_row|, s), s = the median over the output's rows of max|want_row| (row_err): the fp64 gradient
of some rows is zero or tiny by construction (dq of a one-key row is exactly 0), and an error there counts against a typical row.  A row whose
denominator is 0 (an all-zero output) has error 0 when it is matched exactly and inf otherwise.  The YARDSTICK of an output is the largest
row error of the fp32 evaluation over all cases of its family -- for the dense block: of the format model over all cases of the operand set;
the code under test never enters it.

Sparse cross attention.  One CSR over S = 203 keys (S % 4 == 3: the last block of the key pass has an idle wave), R = 34 rows: the lengths
SP_LENGTHS ascending, then descending, so that rows 0 and R - 1 are the empty ones and a row of every length lies in both halves of the launch.
Every non-empty row lists key S - 1 (SP_SHARED_KEY, 32 pairs); keys 1, 2, 3, 4, 5 have exactly 1, 3, 4, 5, 9 pairs (SP_PAIR_COUNTS); keys
100 .. 107 and 201 (SP_UNUSED_KEYS: two whole blocks of the key pass, and the neighbour of key S - 1) have none; the other keys, key 0 among them,
fill the rows in a shuffled order (col_idx is not sorted inside a row).  A 203-key row over 194 keys in use lists some keys twice: the kernels
treat a pair, not a key, as the unit, and so do the references.  q is unit variance / sqrt(32), K and V are bf16 values (exact in every dtype);
'sharp' has q three times as large (the running maximum moves between chunks and waves).  Dropout: ops.attn_drop_mask restated (sp_drop_mask).

Dense block.  One pool of unit-variance q (x 0.3; 'sharp': x 0.9), k, v, dctx; a size means the first n rows / nk keys.  DENSE_CASES: every
n of DENSE_N with every nk of DENSE_NK at p = 0; at p = 0.25 all nk at n = 17 and all n at nk = 33 and 257.  The kernels compute every product
on bf16 hi + lo pairs (mfma3: a_hi b_hi + a_lo b_hi + a_hi b_lo), so their yardstick is the format model Bf16x3: operands rounded to fp32 and
split as split8 of csrc/dense_attn.hip, the three partial products and everything else in fp64.

Denoising self attention: DN_CASES (R, dn_pad, dn_single); a key is visible iff key >= dn_pad, or query < dn_pad and key / dn_single ==
query / dn_single.

Reductions: LayerNorm backward over the first M rows of a pool, rows 0 and M - 1 constant (1.5 and -0.75: a sum of 256 of them is exact in
fp32 in any order, so mean, variance 0 and xhat = 0 are exact in every evaluation); column sums of the first rows x cols of a pool at
ld = cols and cols + 3; the softmax backward on SM_ROWS rows with sentinel pad columns.

Mutants (reference side, fp64): see MUTANTS.  tests/test_train_cases_cpu.py shows each to move some row by >= 3 x cap yardsticks."""
import functools
import math
import types

import numpy as np
import torch

C, HEADS, HD = 256, 8, 32
SEED = 7300
F64, F32 = torch.float64, torch.float32
LN2 = math.log(2.0)

MUTANTS = ('drop_last',        # a row's last key dropped (sparse, dense, denoising self attention)
           'dup_last',         # a row's last key counted twice: what an unmasked clamped key does (its logit + ln 2)
           'mask_nk',          # dense: the backward's dropout mask taken with nk in place of nkp = nk rounded up to 32
           'mask_shift',       # sparse: the backward's dropout mask taken with the pair index shifted by one
           'kv_last_pair',     # sparse: a key's last pair missing from dK / dV
           'drop_lo',          # dense: one lo product dropped in the format model (Bf16x3(drop='a_lo' | 'b_lo'))
           'no_mean_g',        # LayerNorm backward: the mean(g) term missing
           'chunk_last_row',   # column sum: the last row of every 512-row chunk missing
           'rowsum_ld')        # softmax backward: the row sum taken over ld instead of cols

# Bounds of tests/test_gpu_train_edges.py (and of the per-row checks of test_sparse_xattn_backward and test_dense_block_without_materialised_logits):
# per row, kernel error <= K x yardstick.  K = twice the largest ratio measured on an MI355X for the family (profiles/train_rows_vs_fp64.txt),
# rounded up to a power of two; CAP is what tests/test_train_cases_cpu.py shows the cases can carry (every mutant moves some row by >= 3 x CAP
# yardsticks): a ratio beyond the cap is a finding about the kernel, not a reason to raise K.
CAP = dict(sparse_fwd=64.0, sparse_bwd=64.0, dense_fwd=64.0, dense_bwd=64.0, self_attn_dn=64.0, ln_bwd=64.0, colsum=64.0, softmax_bwd=64.0)
K = dict(sparse_fwd=4.0,        # largest measured ratio 1.02 (out of test_sparse_xattn_backward, R = 301; 0.65 on the edge cases)
         sparse_bwd=4.0,        # 1.68 (dK of test_sparse_xattn_backward, R = 37; 1.23 on the edge cases: dq, plain, p = 0.1, 4 waves per query)
         dense_fwd=4.0,         # 1.03 (ctx of test_dense_block_without_materialised_logits, 64 x 128; 1.01 on the edge cases: lse, sharp, 33 x 33)
         dense_bwd=4.0,         # 1.19 (dk of test_dense_block_without_materialised_logits, 400 x 1501; 1.06 on the edge cases: dq, 33 x 257, p = 0.25)
         self_attn_dn=2.0,      # 0.76 (impl 'f32', (65, 48, 3))
         ln_bwd=4.0,            # 1.27 (db, M = 65; dx 1.01, dw 0.85, y 0.87)
         colsum=1.0,            # 0.38 (64 rows, one column, added to a vector)
         softmax_bwd=2.0)       # 0.56 (255 columns, dropped copy)


def _gen(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _randn(seed, shape, scale=1.0):
    return torch.from_numpy((_gen(seed).standard_normal(shape) * scale).astype(np.float32))


# ------------------------------------------------------------------------------------------------ row error
def row_err(got, want, mag=None):
    """[rows] fp64: per row max|got - want| / max(max|want_row|, median over the rows of max|want_row|); a 1-D output is one column per row.
    A NaN in `got` gives a NaN error, which fails every comparison.  mag (same shape as want): the output with its cancelling terms summed by
    magnitude.  It is used only where the WHOLE output vanishes to fp64 rounding (every row's denominator <= 2^-40 of its magnitude: dq and dk of
    a dense block with one key), where the median floor is itself rounding noise: the denominator is then the median row maximum of mag."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.shape[0] == 0:
        return torch.zeros(0, dtype=F64)
    num = (got - want).abs().reshape(want.shape[0], -1).amax(1)
    top = want.abs().reshape(want.shape[0], -1).amax(1)
    den = torch.maximum(top, top.median())
    if mag is not None:
        mtop = mag.detach().double().cpu().abs().reshape(want.shape[0], -1).amax(1)
        if bool((den <= 2.0 ** -40 * mtop).all()):
            den = mtop.median().expand_as(den)
    err = num / den.clamp_min(1e-300)
    return torch.where(den > 0, err, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float('inf'))))


def vec_err(got, want):
    """fp64 scalar: max|got - want| / max|want| of a vector (dw, db, column sums); 0 / 0 = 0, x / 0 = inf"""
    got, want = got.detach().double().cpu().flatten(), want.detach().double().cpu().flatten()
    if want.numel() == 0:
        return 0.0
    num, den = float((got - want).abs().max()), float(want.abs().max())
    if num != num:
        return float('nan')
    return num / den if den > 0 else (0.0 if num == 0 else float('inf'))


def worst(got, want, skip=(), mag=None):
    """largest row error over the rows not in `skip`"""
    e = row_err(got, want, mag)
    if len(skip):
        e = e.clone()
        e[list(skip)] = 0.0
    return float(e.nan_to_num(float('inf')).max()) if e.numel() else 0.0


# ------------------------------------------------------------------------------------------------ sparse cross attention
SP_S = 203
SP_LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 203)
SP_ROW_LENGTHS = SP_LENGTHS + SP_LENGTHS[::-1]
SP_R = len(SP_ROW_LENGTHS)
SP_EMPTY_ROWS = (0, SP_R - 1)
SP_SHARED_KEY = SP_S - 1
SP_PAIR_COUNTS = {1: 1, 2: 3, 3: 4, 4: 5, 5: 9}                      # key -> its exact number of pairs
SP_UNUSED_KEYS = tuple(range(100, 108)) + (201,)
SP_DROPS = (0.0, 0.1, 0.5)
SP_SEED = 123456789


@functools.lru_cache(maxsize=None)
def sp_csr():
    """(row_ptr [R+1] int32, col_idx [nnz] int32)"""
    g = _gen(SEED)
    pool = np.array([k for k in range(SP_S) if k != SP_SHARED_KEY and k not in SP_PAIR_COUNTS and k not in SP_UNUSED_KEYS])
    big = [r for r, n in enumerate(SP_ROW_LENGTHS) if n >= 15]
    special, at = {}, 0
    for key, cnt in SP_PAIR_COUNTS.items():                          # the keys with an exact pair count: one each in `cnt` of the rows of >= 15 keys
        for r in big[at:at + cnt]:
            special[r] = key
        at += cnt
    assert at == len(big) == 22
    rows = []
    for r, n in enumerate(SP_ROW_LENGTHS):
        if n == 0:
            rows.append([])
            continue
        own = [SP_SHARED_KEY] + ([special[r]] if r in special else [])
        need = n - len(own)
        keys = list(g.permutation(pool)[:min(need, len(pool))])
        if need > len(pool):
            keys += list(g.choice(pool, need - len(pool), replace=False))          # a 203-key row: some keys twice
        keys = np.array(own + keys)
        rows.append(list(keys[g.permutation(n)]))
    row_ptr = np.concatenate([[0], np.cumsum([len(x) for x in rows])])
    col = np.concatenate([np.array(x, dtype=np.int64) for x in rows])          # (a 203-key row lists the whole pool, key 0 included)
    return torch.tensor(row_ptr, dtype=torch.int32), torch.tensor(col, dtype=torch.int32)


def sp_drop_mask(nnz, seed, p_drop, shift=0):
    """[nnz, 8] keep / scale factors of pair e, head h: the counter hash of (seed, 8 (e + shift) + h), ops.attn_drop_mask restated"""
    if p_drop <= 0:
        return np.ones((nnz, 8), np.float32)
    pf = np.float32(p_drop)
    t = float(pf) * 4294967296.0
    thr = (0xffffffff if t >= 4294967295.0 else int(t)) or 1
    with np.errstate(over='ignore'):
        u = ((np.arange(nnz * 8, dtype=np.uint64) + np.uint64(8 * shift)) * np.uint64(0x9E3779B1)).astype(np.uint32) ^ np.uint32(seed & 0xffffffff)
        u ^= u >> np.uint32(16); u = (u.astype(np.uint64) * np.uint64(0x85EBCA6B)).astype(np.uint32)
        u ^= u >> np.uint32(13); u = (u.astype(np.uint64) * np.uint64(0xC2B2AE35)).astype(np.uint32)
        u ^= u >> np.uint32(16)
    return np.where(u >= np.uint32(thr), np.float32(1.0) / (np.float32(1.0) - pf), np.float32(0)).reshape(nnz, 8)


@functools.lru_cache(maxsize=None)
def sp_case(kind):
    assert kind in ('plain', 'sharp')
    row_ptr, col = sp_csr()
    q = _randn(SEED + 1, (SP_R, C), 1.0 / math.sqrt(HD)) * (3.0 if kind == 'sharp' else 1.0)
    K, V = (_randn(SEED + i, (SP_S, C)).to(torch.bfloat16) for i in (2, 3))
    return types.SimpleNamespace(kind=kind, row_ptr=row_ptr, col_idx=col, q=q, K=K, V=V, dctx=_randn(SEED + 4, (SP_R, C)), R=SP_R, S=SP_S,
                                 nnz=int(col.numel()), nk=(row_ptr[1:] - row_ptr[:-1]).tolist())


def sp_attend(kind, p_drop=0.0, dtype=F64, mutant=None):
    """ctx, dq [R,256], dK, dV [S,256] of the case: per row and head p = softmax over the row's pairs, ctx = sum_j p_j m_j v_j; dp_j = m_j dctx.v_j,
    ds_j = p_j (dp_j - sum_i p_i dp_i), dq = sum_j ds_j k_j, dK[key_j] += ds_j q, dV[key_j] += p_j m_j dctx.  An empty row has ctx = dq = 0."""
    assert mutant in (None, 'drop_last', 'dup_last', 'mask_shift', 'kv_last_pair')
    c = sp_case(kind)
    rp, col = c.row_ptr.tolist(), c.col_idx.long()
    t = lambda a: a.to(dtype)
    q, Kd, Vd, g = t(c.q).view(-1, HEADS, HD), t(c.K.float()).view(-1, HEADS, HD), t(c.V.float()).view(-1, HEADS, HD), t(c.dctx).view(-1, HEADS, HD)
    mf = torch.from_numpy(sp_drop_mask(c.nnz, SP_SEED, p_drop).astype(np.float64)).to(dtype)
    mb = torch.from_numpy(sp_drop_mask(c.nnz, SP_SEED, p_drop, 1).astype(np.float64)).to(dtype) if mutant == 'mask_shift' else mf
    last_of_key = torch.zeros(c.nnz, dtype=torch.bool)
    if mutant == 'kv_last_pair':
        for s in col.unique().tolist():                              # the pair with the highest id: the last one the key pass walks
            last_of_key[int((col == s).nonzero().max())] = True
    ctx, dq = torch.zeros((c.R, HEADS, HD), dtype=dtype), torch.zeros((c.R, HEADS, HD), dtype=dtype)
    dK, dV = torch.zeros((c.S, HEADS, HD), dtype=dtype), torch.zeros((c.S, HEADS, HD), dtype=dtype)
    for r in range(c.R):
        a, b = rp[r], rp[r + 1]
        if mutant == 'drop_last' and b - a >= 2:
            b -= 1
        if b <= a:
            continue
        cols = col[a:b]
        Kc, Vc = Kd[cols], Vd[cols]                                  # [n,8,32]
        lg = torch.einsum('hd,nhd->nh', q[r], Kc)
        if mutant == 'dup_last':
            lg[-1] += LN2
        P = torch.softmax(lg, 0)
        Pd = P * mf[a:b]
        ctx[r] = torch.einsum('nh,nhd->hd', Pd, Vc)
        dP = torch.einsum('hd,nhd->nh', g[r], Vc) * mb[a:b]
        dS = P * (dP - (P * dP).sum(0, keepdim=True))
        dq[r] = torch.einsum('nh,nhd->hd', dS, Kc)
        keep = (~last_of_key[a:b]).to(dtype)[:, None, None]
        dK.index_add_(0, cols, dS[:, :, None] * q[r][None] * keep)
        dV.index_add_(0, cols, (P * mb[a:b])[:, :, None] * g[r][None] * keep)
    return types.SimpleNamespace(ctx=ctx.reshape(c.R, C), dq=dq.reshape(c.R, C), dK=dK.reshape(c.S, C), dV=dV.reshape(c.S, C))


@functools.lru_cache(maxsize=None)
def sp_refs(kind, p_drop, dtype=F64):
    return sp_attend(kind, p_drop, dtype)


SP_OUTPUTS = ('ctx', 'dq', 'dK', 'dV')


def sp_skip(name):
    """the rows that leave the per-row comparison of a sparse output for an exact check: empty rows (ctx, dq), unused keys (dK, dV)"""
    return SP_EMPTY_ROWS if name in ('ctx', 'dq') else SP_UNUSED_KEYS


@functools.lru_cache(maxsize=None)
def sp_yard(name):
    """the largest row error of the fp32 evaluation over both operand sets and every dropout rate"""
    return max(worst(getattr(sp_refs(k, p, F32), name), getattr(sp_refs(k, p), name)) for k in ('plain', 'sharp') for p in SP_DROPS)


# ------------------------------------------------------------------------------------------------ products of the dense block
class Plain:
    """a product as torch evaluates it in the dtype of its left operand"""

    def __call__(self, expr, a, b):
        return torch.einsum(expr, a, b.to(a.dtype))


def split_bf16(x):
    """fp32 -> (hi, lo) bf16 with x ~ hi + lo: split8 of csrc/dense_attn.hip (round to nearest even, lo = bf16(x - hi))"""
    x = x.float()
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


class Bf16x3:
    """a product on bf16 pairs in fp64: a_hi b_hi + a_lo b_hi + a_hi b_lo (mfma3; lo x lo is what the format leaves out), both operands rounded to
    fp32 first; drop = 'a_lo' | 'b_lo' loses that lo operand's product (the mutants)"""

    def __init__(self, drop=None):
        assert drop in (None, 'a_lo', 'b_lo')
        self.drop = drop

    def __call__(self, expr, a, b):
        (ah, al), (bh, bl) = split_bf16(a), split_bf16(b)
        ah, al, bh, bl = ah.double(), al.double(), bh.double(), bl.double()
        out = torch.einsum(expr, ah, bh)
        if self.drop != 'a_lo':
            out = out + torch.einsum(expr, al, bh)
        if self.drop != 'b_lo':
            out = out + torch.einsum(expr, ah, bl)
        return out


# ------------------------------------------------------------------------------------------------ dense block
DENSE_N = (1, 15, 16, 17, 33)
DENSE_NK = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257)
DENSE_P = 0.25
DENSE_SEED = 1234
DENSE_CASES = tuple((n, nk, 0.0) for n in DENSE_N for nk in DENSE_NK) + tuple(sorted(
    {(17, nk, DENSE_P) for nk in DENSE_NK} | {(n, nk, DENSE_P) for n in DENSE_N for nk in (33, 257)}))
DENSE_OUTPUTS = ('ctx', 'lse', 'dq', 'dk', 'dv')


@functools.lru_cache(maxsize=None)
def dense_pool(kind):
    assert kind in ('plain', 'sharp')
    n, nk = max(DENSE_N), max(DENSE_NK)
    return types.SimpleNamespace(q=_randn(SEED + 10, (n, C), 0.3) * (3.0 if kind == 'sharp' else 1.0), k=_randn(SEED + 11, (nk, C)), v=_randn(SEED + 12, (nk, C)),
                                 go=_randn(SEED + 13, (n, C)))


def dense_drop_mask(n, nk, p, seed, nkp=None):
    """keep / scale factors [8, n, nk] of mv2d_dense_attn_* (csrc/dense_attn.hip: murmur3 finaliser of the counter (head n + query) nkp + key,
    nkp = nk rounded up to 32)"""
    if p <= 0:
        return np.ones((8, n, nk), np.float64)
    nkp = (nk + 31) & ~31 if nkp is None else nkp
    pf = np.float32(p)
    t = float(pf) * 4294967296.0
    thr = (0xffffffff if t >= 4294967295.0 else int(t)) or 1
    idx = ((np.arange(8)[:, None, None] * n + np.arange(n)[None, :, None]) * nkp + np.arange(nk)[None, None, :]).astype(np.uint64)
    with np.errstate(over='ignore'):
        u = ((idx * np.uint64(0x9E3779B1)) & np.uint64(0xffffffff)).astype(np.uint32) ^ np.uint32(seed & 0xffffffff)
        u ^= u >> np.uint32(16); u = ((u.astype(np.uint64) * np.uint64(0x85EBCA6B)) & np.uint64(0xffffffff)).astype(np.uint32)
        u ^= u >> np.uint32(13); u = ((u.astype(np.uint64) * np.uint64(0xC2B2AE35)) & np.uint64(0xffffffff)).astype(np.uint32)
        u ^= u >> np.uint32(16)
    return np.where(u >= np.uint32(thr), np.float32(1.0) / (np.float32(1.0) - pf), np.float32(0.0)).astype(np.float64)


def dense_attend(n, nk, p=0.0, kind='plain', dtype=F64, prod=None, mutant=None, operands=None):
    """ctx [n,256], lse [n,8], dq [n,256], dk, dv [nk,256] of the first n queries and nk keys: S = q k^T per head, P = exp(S - lse), Pd = P m,
    ctx = Pd v; dPd = dO v^T, D = dO . ctx, dS = P (dPd m - D), dq = dS k, dk = dS^T q, dv = Pd^T dO.  The five products go through `prod`.
    operands: (q, k, v, go) in place of the pool's."""
    assert mutant in (None, 'drop_last', 'dup_last', 'mask_nk')
    prod = prod or Plain()
    o = dense_pool(kind)
    q, k, v, go = operands if operands is not None else (o.q[:n], o.k[:nk], o.v[:nk], o.go[:n])
    q, k, v, go = (t.to(dtype).view(-1, HEADS, HD) for t in (q, k, v, go))
    mf = torch.from_numpy(dense_drop_mask(n, nk, p, DENSE_SEED)).to(dtype)
    mb = torch.from_numpy(dense_drop_mask(n, nk, p, DENSE_SEED, nkp=nk)).to(dtype) if mutant == 'mask_nk' else mf
    keys = slice(0, nk - 1) if (mutant == 'drop_last' and nk >= 2) else slice(0, nk)
    S = prod('nhd,mhd->hnm', q, k[keys])
    if mutant == 'dup_last':
        S[:, :, -1] += LN2
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    Pd = P * mf[:, :, keys]
    ctx = prod('hnm,mhd->nhd', Pd, v[keys])
    dPd = prod('nhd,mhd->hnm', go, v[keys])
    D = (go * ctx).sum(-1).transpose(0, 1)                            # [h,n]
    dS = P * (dPd * mb[:, :, keys] - D[..., None])
    dq = prod('hnm,mhd->nhd', dS, k[keys])
    dk, dv = torch.zeros_like(k), torch.zeros_like(v)
    dk[keys] = prod('hnm,nhd->mhd', dS, q)
    dv[keys] = prod('hnm,nhd->mhd', P * mb[:, :, keys], go)
    T = (P * ((dPd * mb[:, :, keys]).abs() + D.abs()[..., None])).double()          # dS with its two terms taken by magnitude (row_err's mag)
    dq_mag = torch.einsum('hnm,mhd->nhd', T, k[keys].double().abs())
    dk_mag = torch.zeros_like(k, dtype=F64)
    dk_mag[keys] = torch.einsum('hnm,nhd->mhd', T, q.double().abs())
    return types.SimpleNamespace(ctx=ctx.reshape(n, C), lse=lse.transpose(0, 1).contiguous(), dq=dq.reshape(n, C), dk=dk.reshape(nk, C), dv=dv.reshape(nk, C),
                                 dq_mag=dq_mag.reshape(n, C), dk_mag=dk_mag.reshape(nk, C))


def dense_mag(ref, name):
    return getattr(ref, name + '_mag') if name in ('dq', 'dk') else None


@functools.lru_cache(maxsize=None)
def dense_refs(n, nk, p, kind='plain'):
    return dense_attend(n, nk, p, kind)


@functools.lru_cache(maxsize=None)
def dense_model(n, nk, p, kind='plain'):
    return dense_attend(n, nk, p, kind, prod=Bf16x3())


def dense_kinds(n, nk, p):
    """the operand sets a case runs on: 'sharp' where the key tiles of a row are dealt to more than one wave or the last tile is ragged"""
    return ('plain', 'sharp') if nk in (33, 129, 257) else ('plain',)


@functools.lru_cache(maxsize=None)
def dense_yard(name, kind='plain'):
    """the largest row error of the format model over every case of the operand set (one yardstick per output and operand set: with the sharp
    logits dS = P (dPd m - D) cancels harder, and the format's error in dk of a single sharp query is six times that of any plain case)"""
    return max(worst(getattr(dense_model(n, nk, p, kind), name), getattr(dense_refs(n, nk, p, kind), name), mag=dense_mag(dense_refs(n, nk, p, kind), name))
               for n, nk, p in DENSE_CASES if kind in dense_kinds(n, nk, p))


# ------------------------------------------------------------------------------------------------ denoising self attention
DN_CASES = ((33, 0, 1), (33, 33, 11), (48, 32, 16), (49, 34, 17), (50, 30, 15), (17, 16, 1), (65, 48, 3))


@functools.lru_cache(maxsize=None)
def dn_qkv(R):
    return _randn(SEED + 20 + R, (R, 3 * C))


def dn_visible(R, dn_pad, dn_single):
    """[R,R] bool: key visible to query (prepare_for_dn's attn_mask, negated)"""
    i = torch.arange(R)
    s = max(dn_single, 1)
    return (i[None, :] >= dn_pad) | ((i[:, None] < dn_pad) & (i[None, :] // s == i[:, None] // s))


def dn_attend(R, dn_pad, dn_single, dtype=F64, mutant=None):
    """[R,256]: softmax over the visible keys of q k^T / sqrt(32), times v, per head"""
    assert mutant in (None, 'drop_last', 'dup_last')
    q, k, v = (t.to(dtype).view(R, HEADS, HD).transpose(0, 1) for t in dn_qkv(R).split(C, 1))
    vis = dn_visible(R, dn_pad, dn_single)
    lg = (q @ k.transpose(1, 2)) / math.sqrt(HD)
    if mutant:
        last = (vis * torch.arange(1, R + 1)[None, :]).argmax(1)      # a row's last visible key
        many = vis.sum(1) >= 2
        for r in range(R):
            if mutant == 'drop_last' and bool(many[r]):
                vis[r, last[r]] = False
            if mutant == 'dup_last':
                lg[:, r, last[r]] += LN2
    lg = lg.masked_fill(~vis[None], float('-inf'))
    return (torch.softmax(lg, -1) @ v).transpose(0, 1).reshape(R, C)


@functools.lru_cache(maxsize=None)
def dn_refs(R, dn_pad, dn_single, dtype=F64):
    return dn_attend(R, dn_pad, dn_single, dtype)


@functools.lru_cache(maxsize=None)
def dn_yard():
    return max(worst(dn_refs(*c, F32), dn_refs(*c)) for c in DN_CASES)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
LN_M = (0, 1, 3, 4, 5, 63, 64, 65, 129)
LN_EPS = 1e-5
LN_CONST = (1.5, -0.75)


@functools.lru_cache(maxsize=None)
def ln_case(M):
    """x, dy [M,256] (rows 0 and M - 1 of x constant), w, b [256]"""
    x = (_randn(SEED + 30, (max(LN_M), C)) * 3.0 + 0.5)[:M].clone()
    if M:
        x[M - 1] = LN_CONST[1]
        x[0] = LN_CONST[0]
    w = torch.from_numpy((_gen(SEED + 31).random(C) + 0.5).astype(np.float32))
    return types.SimpleNamespace(x=x, dy=_randn(SEED + 32, (max(LN_M), C))[:M].clone(), w=w, b=_randn(SEED + 33, (C,)), M=M)


def ln_bwd(M, dtype=F64, mutant=None):
    """y, dx [M,256], dw, db [256]: xhat = (x - mean) rstd, g = dy w, dx = rstd (g - mean(g) - xhat mean(g xhat)), dw = sum dy xhat, db = sum dy"""
    assert mutant in (None, 'no_mean_g')
    c = ln_case(M)
    x, dy, w, b = (t.to(dtype) for t in (c.x, c.dy, c.w, c.b))
    mean = x.mean(1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + LN_EPS)
    xh = xc * rstd
    g = dy * w
    mg = 0.0 if mutant == 'no_mean_g' else g.mean(1, keepdim=True)
    dx = rstd * (g - mg - xh * (g * xh).mean(1, keepdim=True))
    return types.SimpleNamespace(y=xh * w + b, dx=dx, dw=(dy * xh).sum(0), db=dy.sum(0))


@functools.lru_cache(maxsize=None)
def ln_refs(M, dtype=F64):
    return ln_bwd(M, dtype)


@functools.lru_cache(maxsize=None)
def ln_yard(name):
    f = worst if name in ('y', 'dx') else vec_err
    return max(f(getattr(ln_refs(M, F32), name), getattr(ln_refs(M), name)) for M in LN_M)


# ------------------------------------------------------------------------------------------------ column sum
CS_ROWS = (0, 1, 15, 16, 17, 63, 64, 65, 1024, 1025, 1537)
CS_COLS = (1, 10, 16, 17, 256)
CS_PAD = 3
CS_CHUNK = 512


@functools.lru_cache(maxsize=None)
def cs_pool():
    """x [1537, 259] and an `add` vector [256]; a case reads the first rows x (cols | cols + 3) block"""
    return _randn(SEED + 40, (max(CS_ROWS), max(CS_COLS) + CS_PAD)), _randn(SEED + 41, (max(CS_COLS),))


def colsum(rows, cols, dtype=F64, add=False, mutant=None):
    assert mutant in (None, 'chunk_last_row')
    x, a = cs_pool()
    x = x[:rows, :cols].to(dtype)
    if mutant and rows:
        keep = torch.ones(rows, dtype=torch.bool)
        keep[CS_CHUNK - 1::CS_CHUNK] = False
        keep[rows - 1] = False
        x = x[keep]
    s = x.sum(0)
    return s + a[:cols].to(dtype) if add else s


@functools.lru_cache(maxsize=None)
def cs_yard():
    return max(vec_err(colsum(r, c, F32, add), colsum(r, c, F64, add)) for r in CS_ROWS for c in CS_COLS for add in (False, True))


# ------------------------------------------------------------------------------------------------ softmax backward
SM_COLS = (1, 255, 256, 257, 1000)
SM_PAD = 5
SM_ROWS = 5
SM_P = 0.25
SM_SENTINEL = -12345.0


@functools.lru_cache(maxsize=None)
def sm_case(cols, padded, dropped):
    """P, Pd, dP [5, ld] fp32 with ld = cols (+ 5 pad columns that hold the sentinel in all three), keep_scale"""
    ld = cols + (SM_PAD if padded else 0)
    P = torch.softmax(_randn(SEED + 50 + cols, (SM_ROWS, cols), 2.0).double(), 1).float()
    dP = _randn(SEED + 51 + cols, (SM_ROWS, cols))
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(SM_P))) if dropped else 1.0
    keep = torch.from_numpy(_gen(SEED + 52 + cols).random((SM_ROWS, cols)) >= SM_P) if dropped else torch.ones((SM_ROWS, cols), dtype=torch.bool)
    full = lambda t: torch.cat([t, torch.full((SM_ROWS, ld - cols), SM_SENTINEL)], 1).contiguous()
    return types.SimpleNamespace(P=full(P), Pd=full(P * keep * scale), dP=full(dP), ld=ld, cols=cols, keep_scale=scale, dropped=dropped)


def softmax_bwd(cols, padded, dropped, dtype=F64, mutant=None):
    """dS [5, cols] = P (dP m - sum_j P_j dP_j m_j), m = keep_scale where Pd != 0 else 0"""
    assert mutant in (None, 'rowsum_ld')
    c = sm_case(cols, padded, dropped)
    w = c.ld if mutant == 'rowsum_ld' else cols
    P, dP = c.P.to(dtype), c.dP.to(dtype)
    m = (c.Pd != 0).to(dtype) * c.keep_scale
    r = (P[:, :w] * dP[:, :w] * m[:, :w]).sum(1, keepdim=True)
    return (P * (dP * m - r))[:, :cols]


@functools.lru_cache(maxsize=None)
def sm_yard():
    return max(worst(softmax_bwd(c, pad, dr, F32), softmax_bwd(c, pad, dr)) for c in SM_COLS for pad in (False, True) for dr in (False, True))
