"""Cases and plain torch references for the row side of a decoder layer: the row-block kernels of csrc/rowblock.hip (ops.attn_out_fused_x3,
ops.attn_out_qmap_x3, ops.attn_out_zmap_x3, ops.ffn_out_fused_x3) and the self-attention core (csrc/self_attn_x3.hip, csrc/attention.hip through
ops.self_attn).  No tests here: tests/test_rowblock_cases_cpu.py shows on the CPU that the cases tell a correct fp32-class kernel from one that
loses a lo product or mishandles a sample's last key, tests/test_gpu_rowblock_edges.py holds the kernels to them.  Needs neither the library
nor a GPU; qk_map, split_key16 and row_errors are those of tests/xattn_cases.py.

Row operands (one set of M_ALL = 545 rows, in the style of test_attn_out_fused_x3 / test_ffn_out_fused_x3 of tests/test_gpu_kernels.py):
unit-variance ctx, resid, qpos [545,256] and z [545,8,256]; 256 x 256 weights of scale 0.06 (Wo, Wq of the out-projection and the cross
attention's q projection, Wk, Wv of the per-head maps), the self-attention in-projection Win [768,256] (rows 0..255 | 256..511 | 512..767 are
its Wq | Wk | Wv) of the same scale; unit-variance biases and LayerNorm parameters; FFN slabs parts [32,545,256] of scale 0.3 (a launch with
n_parts slabs reads the first n_parts).  A row count M of ROW_COUNTS always means the FIRST M rows:
    1, 16, 17       one row, one full 16-row tile, one row behind it
    512             the last launch with 16 rows per block (RT = 1)
    513             32 rows per block (RT = 2), one row in the last block
    528             RT = 2, the second tile of the last block empty
    529             RT = 2, one row in that second tile
    545             17 full blocks of 32 rows plus one row
The CSR row_ptr gives every row 1 .. 5 keys except EMPTY_ROWS = 0, 15, 16, 511, 512, 527, 528, 544 (first and last row of a tile, of the
RT = 1 range, of the last block's tiles at M = 528 / 529 / 545); the context map reads only the differences of adjacent entries.

References, each a function of dtype (float64: the reference; float32: the plain torch evaluation whose largest per-row error is the yardstick):
    attn_chain   x = LN(ctx Wo^T + bo + resid), q = ((x + qpos) Wq^T + bq) QSCALE, Qt = qk_map(q, Wk)
    zmap_chain   ctx[:, 32 h + d] = sum_c Wv[32 h + d, c] z[:, h, c] + bv, an empty row replaced AFTER the bias by NaN (empty_nan) or 0 (not
                 bv), then the same x
    tail_chain   y = LN(sum_s parts[s] + b2 + resid) summed in the order s = 0, 1, ..., xq = y + qpos, outs = post_norm(y),
                 qkv = [xq Wq^T | xq Wk^T | y Wv^T] + b_in with the three blocks of Win
Every product goes through one callable (Plain: torch.einsum in the dtype).  Q16Model is the format model of the shipped q16 pairs: a product
is a_hi w_hi + a_lo w_hi + a_hi w_lo on fp16 pairs split like split_q16x2 of csrc/common.h (saturate at +-65504, lo = fp16(x - hi)), the
operand rounded to fp32 first, everything else in fp64; drop='a_lo' / 'w_lo' are the two mutants that lose one lo product.

Self-attention: one batch of samples of SA_SIZES rows (1491 rows, both sides of 16, 32, 64, 128, 256: the query wave, the key step, the query
block, the key chunk and two chunks) with SA_PAD = 40 padding rows behind them; sa_case('plain') has unit-variance qkv (the logits the decoder
produces), sa_case('sharp') the same with q three times as large (the running maximum moves between 32-key steps and 128-key chunks, as in
test_self_attn).  sa_attend is masked softmax attention inside each sample, 8 heads x 32; its mutants drop a sample's last key or count it
twice (what an unmasked clamped padding key does)."""
import functools
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

from xattn_cases import C, HEADS, qk_map, row_errors, split_key16          # noqa: F401  (row_errors: for the two test modules)

M_ALL = 545
ROW_COUNTS = (1, 16, 17, 512, 513, 528, 529, 545)
EMPTY_ROWS = (0, 15, 16, 511, 512, 527, 528, 544)
N_PARTS_ALL = 32
PARTS_COUNTS = (1, 4, 7, 23, 32)                   # 23 = 16 + 4 + 3: the 16-wide, the 4-wide and the single-slab loop of the slab sum
QSCALE = 1.0 / math.sqrt(32.0)                     # ops.SCALE_Q, restated
EPS = 1e-5
SEED = 5100

SA_SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
SA_PAD = 40
SA_SCALE = 1.0 / math.sqrt(32.0)

# The bounds of tests/test_gpu_rowblock_edges.py: per row, kernel error <= K x the largest per-row error of the fp32 evaluation.  Each K is twice
# the largest ratio measured on an MI355X for its family (profiles/rowblock_rows_vs_fp64.txt), rounded up to a power of two; the caps
# (K_ROWS <= 16, K_SA <= 64) are what tests/test_rowblock_cases_cpu.py shows the cases can carry.
K_ROWS = 4.0                                       # largest measured ratio 1.40 (Qt)
K_SA_X3_PLAIN, K_SA_X3_SHARP, K_SA_F32 = 2.0, 2.0, 2.0        # 0.69, 0.60, 0.89
K_SA = max(K_SA_X3_PLAIN, K_SA_X3_SHARP, K_SA_F32)


def _randn(seed, shape, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


@functools.lru_cache(maxsize=None)
def operands():
    s = iter(range(SEED, SEED + 64))
    r = lambda shape, scale=1.0: _randn(next(s), shape, scale)
    o = types.SimpleNamespace(
        ctx=r((M_ALL, C)), resid=r((M_ALL, C)), qpos=r((M_ALL, C)), z=r((M_ALL, HEADS, C)),
        Wo=r((C, C), 0.06), Wq=r((C, C), 0.06), Wk=r((C, C), 0.06), Wv=r((C, C), 0.06), Win=r((3 * C, C), 0.06),
        bo=r((C,)), bq=r((C,)), bv=r((C,)), b2=r((C,)), b_in=r((3 * C,)),
        lw=r((C,)), lb=r((C,)), tw=r((C,)), tb=r((C,)), pw=r((C,)), pb=r((C,)),
        parts=r((N_PARTS_ALL, M_ALL, C), 0.3))
    nk = torch.tensor([0 if m in EMPTY_ROWS else 1 + (7 * m) % 5 for m in range(M_ALL)])
    o.row_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), nk.cumsum(0)]).to(torch.int32)
    o.empty = nk == 0
    return o


# ------------------------------------------------------------------------------------------------ products
class Plain:
    """a product as torch evaluates it in the dtype of its left operand"""

    def __call__(self, expr, a, w):
        return torch.einsum(expr, a, w.to(a.dtype))


def split_q16(x):
    """fp32 -> (hi, lo) fp16 pair of the shipped q16 format: csrc/common.h split_q16x2 (saturate at +-65504, lo = fp16(x - hi); a NaN stays NaN)"""
    return split_key16(x.float().clamp(-65504.0, 65504.0))


class Q16Model:
    """a product on fp16 pairs in fp64: a_hi w_hi + a_lo w_hi + a_hi w_lo (lo x lo is what the format leaves out); drop = 'a_lo' | 'w_lo' loses
    that lo operand's product (the mutants)"""

    def __init__(self, drop=None):
        assert drop in (None, 'a_lo', 'w_lo')
        self.drop = drop

    def __call__(self, expr, a, w):
        (ah, al), (wh, wl) = split_q16(a), split_q16(w)
        ah, al, wh, wl = ah.double(), al.double(), wh.double(), wl.double()
        out = torch.einsum(expr, ah, wh)
        if self.drop != 'a_lo':
            out = out + torch.einsum(expr, al, wh)
        if self.drop != 'w_lo':
            out = out + torch.einsum(expr, ah, wl)
        return out


LIN, QMAP, ZMAP = 'mk,nk->mn', 'rhd,hdc->rhc', 'rhc,hdc->rhd'


def _ln(v, w, b):
    return F.layer_norm(v, (C,), w.to(v.dtype), b.to(v.dtype), EPS)


def _rows(rows):
    return slice(0, rows) if isinstance(rows, int) else rows


# ------------------------------------------------------------------------------------------------ the references
def attn_chain(dtype=torch.float64, rows=M_ALL, prod=None, ctx=None):
    """x [M,256], q [M,256], Qt [M,8,256] of the rows `rows` (a count: the first rows; or a slice); ctx: another context tile for these rows"""
    o, rows, prod = operands(), _rows(rows), prod or Plain()
    t = lambda a: a.to(dtype)
    ctx = t(o.ctx[rows]) if ctx is None else ctx
    x = _ln(prod(LIN, ctx, o.Wo) + t(o.bo) + t(o.resid[rows]), o.lw, o.lb)
    q = (prod(LIN, x + t(o.qpos[rows]), o.Wq) + t(o.bq)) * QSCALE
    if isinstance(prod, Plain):
        Qt = qk_map(q, o.Wk) if dtype == torch.float64 else prod(QMAP, q.view(-1, HEADS, 32), o.Wk.view(HEADS, 32, C))
    else:
        hi, lo = split_key16(prod(QMAP, q.view(-1, HEADS, 32), o.Wk.view(HEADS, 32, C)).float())        # stored as a key16 pair
        Qt = hi.double() + lo.double()
    return types.SimpleNamespace(x=x, q=q, Qt=Qt)


def zmap_chain(dtype=torch.float64, rows=M_ALL, prod=None, empty_nan=True):
    """ctx [M,256] of the context map (empty rows NaN / 0) and x = LN(ctx Wo^T + bo + resid) behind it"""
    o, rows, prod = operands(), _rows(rows), prod or Plain()
    ctx = prod(ZMAP, o.z[rows].to(dtype), o.Wv.view(HEADS, 32, C)).reshape(-1, C) + o.bv.to(dtype)
    ctx[o.empty[rows]] = float('nan') if empty_nan else 0.0
    return types.SimpleNamespace(ctx=ctx, x=attn_chain(dtype, rows, prod, ctx=ctx).x)


def tail_chain(dtype=torch.float64, rows=M_ALL, prod=None, n_parts=N_PARTS_ALL):
    """y, xq, outs [M,256] and qkv [M,768] of the FFN tail over the first n_parts slabs"""
    o, rows, prod = operands(), _rows(rows), prod or Plain()
    t = lambda a: a.to(dtype)
    v = torch.zeros_like(t(o.resid[rows]))
    for s in range(n_parts):
        v = v + t(o.parts[s, rows])
    y = _ln(v + t(o.b2) + t(o.resid[rows]), o.tw, o.tb)
    xq = y + t(o.qpos[rows])
    qkv = torch.cat([prod(LIN, xq, o.Win[:2 * C]), prod(LIN, y, o.Win[2 * C:])], 1) + t(o.b_in)
    return types.SimpleNamespace(y=y, xq=xq, outs=_ln(y, o.pw, o.pb), qkv=qkv)


@functools.lru_cache(maxsize=None)
def attn_refs(dtype):
    return attn_chain(dtype)


@functools.lru_cache(maxsize=None)
def zmap_refs(dtype, empty_nan):
    return zmap_chain(dtype, empty_nan=empty_nan)


@functools.lru_cache(maxsize=None)
def tail_refs(dtype, n_parts=N_PARTS_ALL):
    return tail_chain(dtype, n_parts=n_parts)


def yardstick(f32, f64, rows=None):
    """largest per-row error of the fp32 evaluation against fp64 over the rows `rows` ([M] bool; default all)"""
    e = row_errors(f32, f64)
    return float((e if rows is None else e[rows]).max())


# ------------------------------------------------------------------------------------------------ self-attention
@functools.lru_cache(maxsize=None)
def sa_case(kind):
    assert kind in ('plain', 'sharp')
    R = sum(SA_SIZES)
    qkv = _randn(SEED + 100, (R + SA_PAD, 3 * C))
    if kind == 'sharp':
        qkv[:, :C] *= 3.0
    grp = torch.tensor(np.concatenate([[0], np.cumsum(SA_SIZES)]), dtype=torch.int32)
    return types.SimpleNamespace(kind=kind, qkv=qkv, R=R, sizes=SA_SIZES, grp_start=grp, starts=grp[:-1].tolist())


def sa_attend(case, dtype=torch.float64, mutant=None):
    """[R,256]: softmax(q k^T / sqrt(32)) v per sample and head.  mutant: 'drop_last' (the sample's last key missing) | 'dup_last' (counted
    twice); a one-key sample is left as it is by both"""
    assert mutant in (None, 'drop_last', 'dup_last')
    out = torch.zeros((case.R, C), dtype=dtype)
    for o, n in zip(case.starts, case.sizes):
        q, k, v = (t.to(dtype).view(n, HEADS, 32).transpose(0, 1) for t in case.qkv[o:o + n].split(C, 1))
        if n >= 2 and mutant == 'drop_last':
            k, v = k[:, :-1], v[:, :-1]
        if n >= 2 and mutant == 'dup_last':
            k, v = torch.cat([k, k[:, -1:]], 1), torch.cat([v, v[:, -1:]], 1)
        att = torch.softmax((q @ k.transpose(1, 2)) * SA_SCALE, -1)
        out[o:o + n] = (att @ v).transpose(0, 1).reshape(n, C)
    return out


@functools.lru_cache(maxsize=None)
def sa_refs(kind):
    """(case, fp64 reference [R,256], yardstick: the largest per-row error of the fp32 evaluation over ALL rows of the case -- a one-key sample
    has fp32 error 0, so a yardstick per sample would be 0 there)"""
    case = sa_case(kind)
    ref = sa_attend(case)
    return case, ref, float(row_errors(sa_attend(case, torch.float32), ref).max())
