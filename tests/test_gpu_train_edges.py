"""The attention and reduction kernels of the training route at the counts where they change behaviour (-m gpu): the sparse cross attention and
its backward in both key-pass forms (ops.sparse_xattn, mv2d_sparse_xattn_bwd_ex / ops.sparse_xattn_bwd), the dense block of the denoising rows
(mv2d_dense_attn_fwd / mv2d_dense_attn_bwd_parts, FlashDenseAttnFn), the self attention with the denoising mask (ops.self_attn_dn, both impls)
and the row reductions (mv2d_layer_norm_bwd and autograd_ops.layer_norm, mv2d_colsum / mv2d_colsum_add, mv2d_softmax_bwd_rows).  Cases, references,
the format model and the row error: tests/train_cases.py; tests/test_train_cases_cpu.py shows that every mutant of train_cases.MUTANTS moves some
row by >= 3 x CAP = 192 yardsticks, where a yardstick is the largest row error of a plain fp32 evaluation (torch, CPU) of the same operands
against fp64 -- for the dense block, whose products run on bf16 hi + lo pairs, that of the format model.

Which case reaches which edge:
    sparse     rows of 0 .. 5, 15 .. 17, 31 .. 33, 63 .. 65, 97, 203 keys: below one 4-key chunk, one wave's chunk +- 1, one 32-key round of the
               8 waves +- 1, two and three rounds +- 1 (three chunks in flight, indices clamped to end - 1); the query pass with 4 and with 16
               waves (waves without a key merge through exp(-inf)); keys with 0, 1, 3, 4, 5, 9 and 32 pairs in the key pass with one wave per
               key (S = 203: an idle wave in the last block) and with 4 waves per key
    dense      n = 1, 15, 16, 17, 33 (one ragged, one full, two and three 16-query tiles) x nk = 1 .. 257 around the 16-key sub-tile, the 32-key
               tile, the 128 keys of a key-pass block and the 256 keys of a round of the 8 waves
    DN         group boundaries on, before and behind the 16-key tile edges; no denoising rows; no matched rows but one; only denoising rows
    reductions M around the 4 rows of a pass and the 64 rows of a block; column sums around the 16 row groups, the unroll of 4 and the 512-row
               chunks of the two-pass form; softmax rows around the 256 threads
Every output lies in front of a guard of 32 rows filled with a sentinel that must be intact after every launch; dK, dV and the reductions'
outputs are pre-filled with the sentinel, so a zero there was written.

Exact (no tolerance): rows without a key have ctx 0 (all-NaN under empty_nan, and no other row has a NaN) and dq 0; keys without a pair have
dK = dV = 0; dq at dq_scale = 0.5 is half of dq at 1.0 bit for bit; a second call returns the same bits; ops.sparse_xattn_bwd(long_rows=,
dq_scale=) is the raw entry, and long_rows=None the short-row form on these cases; parts = 1 then parts = 2 of the dense backward on one
workspace are the bits of parts = 3, and FlashDenseAttnFn's; with n = 0 the dense backward writes dk = dv = 0; self_attn_dn with dn_pad = 0 is
ops.self_attn bit for bit (both impls); M = 0 gives dw = db = 0, rows = 0 the zero sum or `add`; the pad columns of the softmax backward survive.

Per row against fp64: error <= K x yardstick, one K per family (train_cases.K).  Measured on an MI355X (the lines of -s are
profiles/train_rows_vs_fp64.txt), largest ratio per family and K = twice that, rounded up to a power of two:
    sparse forward    0.65 (ctx, sharp, p = 0.1; 1.02 for the out of test_sparse_xattn_backward at R = 301)                 K = 4
    sparse backward   1.23 (dq, plain, p = 0.1, 4 waves per query; dK 1.09, dV 1.18; 1.68 for dK of test_sparse_xattn_backward)      K = 4
    dense forward     1.01 (lse, sharp, 33 x 33; ctx 1.00; 1.03 for test_dense_block_without_materialised_logits at 64 x 128)        K = 4
    dense backward    1.06 (dq, plain, 33 x 257, p = 0.25; dk 1.00, dv 1.00; 1.19 for dk of that test at 400 x 1501)                 K = 4
    self_attn_dn      0.76 (impl 'f32', (65, 48, 3))                                                                          K = 2
    LayerNorm         1.27 (db, M = 65; dx 1.01, dw 0.85, y 0.87)                                                             K = 4
    column sum        0.38 (64 rows, one column)                                                                              K = 1
    softmax backward  0.56 (255 columns, dropped copy)                                                                        K = 2
The dense block sits at 1.00 x its format model: the three-product format, not the arithmetic around it, is the kernel's whole error.  The
yardsticks are torch's fp32 on the host and move with it (sparse ctx: 5.4e-7 on the GPU host, 7.7e-7 on a build host).
Found: nothing.  No guard was touched, every exact claim held, no row came near its bound; no kernel text changed.
Seen to fail in a scratch build of the library: sparse_xattn_kernel without its `base + i < end` mask (the clamped keys of a row's last chunk
counted again): all 12 cases of test_sparse_forward_rows, ctx at 1.2e6 .. 1.5e6 yardsticks.
These kernels do not use the q16 format: a -DMV2D_Q16_BF16 build runs the same bounds."""
import ctypes
import functools

import pytest
import torch

import train_cases as tc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -12345.0
GUARD_ROWS = 32
F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------ helpers
def _guarded(rows, width, dtype=torch.float32):
    """(buffer, view [rows, width]): the view and GUARD_ROWS rows behind it hold the sentinel"""
    buf = torch.full(((rows + GUARD_ROWS) * width,), SENTINEL, device=DEV, dtype=dtype)
    return buf, buf[:rows * width].view(rows, width)


def _intact(buf, n):
    return bool((buf[n:] == buf.new_tensor(SENTINEL)).all())


def _same_bits(a, b):
    """NaN in the same places, the same bits elsewhere"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a.masked_fill(na, 0.0).view(torch.int32), b.masked_fill(nb, 0.0).view(torch.int32))


@functools.lru_cache(maxsize=None)
def _lib():
    from mv2d_amd import _lib as L
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return L.load()


def _check(rc, what):
    from mv2d_amd import _lib as L
    L.check(rc, what)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    """the address of a tensor's first element -- of an empty view too (data_ptr() of a tensor without elements is null)"""
    return ctypes.c_void_p(t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size())


def _hold(family, tag, what, got, want, yard, skip=(), mag=None, vec=False):
    """the largest row error of `got` (all rows but `skip`; vec: per element against max|want|) against K x the yardstick; one line per output"""
    w = tc.vec_err(got, want) if vec else tc.worst(got, want, skip, mag)
    print(f'train_ratio {family} {tag} {what}: largest {"element" if vec else "row"} error {w:.3e} = {w / yard:.2f} x the yardstick ({yard:.3e})')
    assert w <= tc.K[family] * yard, (family, tag, what, w / yard)            # (a NaN fails the comparison)


# ------------------------------------------------------------------------------------------------ sparse cross attention
@functools.lru_cache(maxsize=None)
def _sp_dev(kind):
    from mv2d_amd import ops
    _lib()
    c = tc.sp_case(kind)
    d = type(c)(**{k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in vars(c).items()})
    d.transposed = ops.csr_transpose(d.row_ptr, d.col_idx, d.S)
    return d


def _sp_fwd(kind, p, empty_nan):
    from mv2d_amd import ops
    d = _sp_dev(kind)
    buf, ctx = _guarded(d.R, 256)
    ops.sparse_xattn(d.q, d.K, d.V, d.row_ptr, d.col_idx, out=ctx, R=d.R, empty_nan=empty_nan, p_drop=p, seed=tc.SP_SEED)
    torch.cuda.synchronize()
    assert _intact(buf, d.R * 256), ('sparse_xattn', kind, p, empty_nan)
    return ctx


def _sp_bwd(kind, p, long_rows, dq_scale=1.0):
    """mv2d_sparse_xattn_bwd_ex into sentinel-filled dq, dK, dV and pair workspace with guards behind; ctx is the forward kernel's"""
    d = _sp_dev(kind)
    ctx = _sp_fwd(kind, p, False)
    key_ptr, pair_idx, pair_row = d.transposed
    (qb, dq), (kb, dK), (vb, dV), (wb, ws) = _guarded(d.R, 256), _guarded(d.S, 256), _guarded(d.S, 256), _guarded(d.nnz, 16)
    _check(_lib().mv2d_sparse_xattn_bwd_ex(_p(d.q), _p(d.K), _p(d.V), _p(d.row_ptr), _p(d.col_idx), _p(ctx), _p(d.dctx), _p(key_ptr), _p(pair_idx),
                                           _p(pair_row), _p(ws), _p(dq), _p(dK), _p(dV), d.R, d.S, float(p), tc.SP_SEED, long_rows, float(dq_scale),
                                           _st()), 'mv2d_sparse_xattn_bwd_ex')
    torch.cuda.synchronize()
    assert _intact(qb, d.R * 256) and _intact(kb, d.S * 256) and _intact(vb, d.S * 256) and _intact(wb, d.nnz * 16), ('sparse_xattn_bwd', kind, p, long_rows)
    return ctx, dq, dK, dV


@pytest.mark.parametrize('empty_nan', [False, True])
@pytest.mark.parametrize('p', tc.SP_DROPS)
@pytest.mark.parametrize('kind', ['plain', 'sharp'])
def test_sparse_forward_rows(kind, p, empty_nan):
    """ctx of every row with a key against fp64; the two empty rows (first and last of the launch) exactly 0, or all-NaN under empty_nan with no
    NaN anywhere else; a second call returns the same bits."""
    ctx = _sp_fwd(kind, p, empty_nan)
    empty = list(tc.SP_EMPTY_ROWS)
    nan_rows = torch.isnan(ctx).cpu()
    if empty_nan:
        assert sorted(nan_rows.all(1).nonzero().flatten().tolist()) == sorted(nan_rows.any(1).nonzero().flatten().tolist()) == sorted(empty)
    else:
        assert not bool(nan_rows.any()) and float(ctx[empty].abs().max()) == 0.0
    assert _same_bits(ctx, _sp_fwd(kind, p, empty_nan))
    _hold('sparse_fwd', f'{kind} p={p} empty_nan={int(empty_nan)}', 'ctx', ctx, tc.sp_refs(kind, p).ctx, tc.sp_yard('ctx'), skip=tc.sp_skip('ctx'))


@pytest.mark.parametrize('long_rows', [0, 1])
@pytest.mark.parametrize('p', tc.SP_DROPS)
@pytest.mark.parametrize('kind', ['plain', 'sharp'])
def test_sparse_backward_rows(kind, p, long_rows):
    """dq of every row and dK, dV of every key against fp64 in both forms of the two passes (4 waves per query and one wave per key; 16 waves per
    query and 4 waves per key), each held to the bound; rows without a key have dq exactly 0, keys without a pair dK = dV exactly 0 (written over
    the sentinel); a second call returns the same bits; dq_scale = 0.5 halves dq bit for bit and leaves dK, dV alone; the wrapper's keywords
    reach the entry."""
    from mv2d_amd import ops
    d = _sp_dev(kind)
    ctx, dq, dK, dV = _sp_bwd(kind, p, long_rows)
    assert float(dq[list(tc.SP_EMPTY_ROWS)].abs().max()) == 0.0
    assert float(dK[list(tc.SP_UNUSED_KEYS)].abs().max()) == 0.0 and float(dV[list(tc.SP_UNUSED_KEYS)].abs().max()) == 0.0
    _, dq2, dK2, dV2 = _sp_bwd(kind, p, long_rows)
    assert _same_bits(dq, dq2) and _same_bits(dK, dK2) and _same_bits(dV, dV2)
    _, dqh, dKh, dVh = _sp_bwd(kind, p, long_rows, dq_scale=0.5)
    assert _same_bits(dqh, dq * 0.5) and _same_bits(dKh, dK) and _same_bits(dVh, dV)
    for scale, want in ((1.0, dq), (0.5, dqh)):
        got = ops.sparse_xattn_bwd(d.q, d.K, d.V, d.row_ptr, d.col_idx, ctx, d.dctx, transposed=d.transposed, p_drop=p, seed=tc.SP_SEED,
                                   long_rows=long_rows, dq_scale=scale)
        assert _same_bits(got[0], want) and _same_bits(got[1], dK) and _same_bits(got[2], dV)
    if long_rows == 0:                                                 # the density heuristic: these short rows take the short-row kernels
        got = ops.sparse_xattn_bwd(d.q, d.K, d.V, d.row_ptr, d.col_idx, ctx, d.dctx, p_drop=p, seed=tc.SP_SEED)
        assert _same_bits(got[0], dq) and _same_bits(got[1], dK) and _same_bits(got[2], dV)
    ref = tc.sp_refs(kind, p)
    for name, got in (('dq', dq), ('dK', dK), ('dV', dV)):
        assert bool(torch.isfinite(got).all()), name
        _hold('sparse_bwd', f'{kind} p={p} long_rows={long_rows}', name, got, getattr(ref, name), tc.sp_yard(name), skip=tc.sp_skip(name))


# ------------------------------------------------------------------------------------------------ dense block
def _ws(n, nk, backward):
    """a workspace of exactly mv2d_dense_attn_ws_bytes with 4 KB of guard bytes behind it"""
    nbytes = int(_lib().mv2d_dense_attn_ws_bytes(n, nk, backward))
    buf = torch.full((nbytes + 4096,), 0xA5, device=DEV, dtype=torch.uint8)
    assert buf.data_ptr() % 256 == 0
    return buf, nbytes


def _ws_intact(buf, nbytes):
    return bool((buf[nbytes:] == 0xA5).all())


@functools.lru_cache(maxsize=None)
def _dense_dev(kind):
    o = tc.dense_pool(kind)
    return type(o)(**{k: v.to(DEV) for k, v in vars(o).items()})


def _dense_fwd(q, k, v, n, nk, p):
    (cb, ctx), (lb, lse) = _guarded(n, 256), _guarded(8, max(n, 1))
    ws, nbytes = _ws(n, nk, 0)
    _check(_lib().mv2d_dense_attn_fwd(_p(q), _p(k), _p(v), n, nk, float(p), tc.DENSE_SEED, _p(ctx), _p(lse), _p(ws), _st()), 'mv2d_dense_attn_fwd')
    torch.cuda.synchronize()
    assert _intact(cb, n * 256) and _intact(lb, 8 * n) and _ws_intact(ws, nbytes), ('dense_attn_fwd', n, nk, p)
    return ctx, lb[:8 * n].view(8, n)


def _dense_bwd(q, k, v, ctx, go, lse, n, nk, p, parts_seq, dq_scale=1.0):
    (qb, dq), (kb, dk), (vb, dv) = _guarded(n, 256), _guarded(nk, 256), _guarded(nk, 256)
    ws, nbytes = _ws(n, nk, 1)
    for parts in parts_seq:
        _check(_lib().mv2d_dense_attn_bwd_parts(_p(q), _p(k), _p(v), _p(ctx), _p(go), _p(lse), n, nk, float(p), tc.DENSE_SEED, float(dq_scale), _p(dq),
                                                _p(dk), _p(dv), _p(ws), parts, _st()), 'mv2d_dense_attn_bwd_parts')
    torch.cuda.synchronize()
    assert _intact(qb, n * 256) and _intact(kb, nk * 256) and _intact(vb, nk * 256) and _ws_intact(ws, nbytes), ('dense_attn_bwd', n, nk, p, parts_seq)
    return dq, dk, dv


@pytest.mark.parametrize('n,nk,p', tc.DENSE_CASES)
def test_dense_block_rows(n, nk, p):
    """ctx, lse and dq of every query and dk, dv of every key against fp64, on the plain operands and (nk = 33, 129, 257) the sharp ones; the
    backward in two parts on one workspace and FlashDenseAttnFn give the bits of the one-call backward."""
    from mv2d_amd.autograd_ops import FlashDenseAttnFn
    _lib()
    for kind in tc.dense_kinds(n, nk, p):
        o = _dense_dev(kind)
        q, k, v, go = o.q[:n].contiguous(), o.k[:nk].contiguous(), o.v[:nk].contiguous(), o.go[:n].contiguous()
        ctx, lse = _dense_fwd(q, k, v, n, nk, p)
        dq, dk, dv = _dense_bwd(q, k, v, ctx, go, lse, n, nk, p, (3,))
        dq2, dk2, dv2 = _dense_bwd(q, k, v, ctx, go, lse, n, nk, p, (1, 2))
        assert _same_bits(dq, dq2) and _same_bits(dk, dk2) and _same_bits(dv, dv2)
        qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
        out = FlashDenseAttnFn.apply(qa, ka, va, p, tc.DENSE_SEED)
        out.backward(go)
        assert _same_bits(out.detach(), ctx) and _same_bits(qa.grad, dq) and _same_bits(ka.grad, dk) and _same_bits(va.grad, dv)
        ref, tag = tc.dense_refs(n, nk, p, kind), f'{kind} n={n} nk={nk} p={p}'
        for name, got in (('ctx', ctx), ('lse', lse.t()), ('dq', dq), ('dk', dk), ('dv', dv)):
            assert bool(torch.isfinite(got).all()), (tag, name)
            _hold('dense_fwd' if name in ('ctx', 'lse') else 'dense_bwd', tag, name, got, getattr(ref, name), tc.dense_yard(name, kind),
                  mag=tc.dense_mag(ref, name))


@pytest.mark.parametrize('nk', [1, 33, 257])
def test_dense_block_without_queries_writes_zero_key_gradients(nk):
    """n = 0: the forward has nothing to write, the backward writes dk = dv = 0 (parts 3 and parts 2) and no dq."""
    o = _dense_dev('plain')
    k, v = o.k[:nk].contiguous(), o.v[:nk].contiguous()
    q = torch.zeros(1, 256, device=DEV)                              # (a non-null pointer for the empty operands)
    for parts_seq in ((3,), (1, 2), (2,)):
        dq, dk, dv = _dense_bwd(q, k, v, q, q, q, 0, nk, 0.25, parts_seq)
        assert float(dk.abs().max()) == 0.0 and float(dv.abs().max()) == 0.0
    dq, dk, dv = _dense_bwd(q, k, v, q, q, q, 0, nk, 0.25, (1,))
    assert bool((dk == SENTINEL).all()) and bool((dv == SENTINEL).all())
    _dense_fwd(q, k, v, 0, nk, 0.25)


# ------------------------------------------------------------------------------------------------ denoising self attention
@pytest.mark.parametrize('impl', ['f32', 'x3'])
@pytest.mark.parametrize('R,dn_pad,dn_single', tc.DN_CASES)
def test_self_attn_dn_rows(R, dn_pad, dn_single, impl):
    """Every row against masked attention in fp64, group boundaries on, before and behind the 16-key tile edges; without denoising rows the
    result is ops.self_attn's bit for bit (both impls: the mask is evaluated in the inference kernels' arithmetic)."""
    from mv2d_amd import ops
    _lib()
    qkv = tc.dn_qkv(R).to(DEV)
    buf, out = _guarded(R, 256)
    ops.self_attn_dn(qkv, dn_pad, dn_single, out=out, impl=impl)
    torch.cuda.synchronize()
    assert _intact(buf, R * 256) and bool(torch.isfinite(out).all())
    _hold('self_attn_dn', f'impl={impl} R={R} dn_pad={dn_pad} dn_single={dn_single}', 'ctx', out, tc.dn_refs(R, dn_pad, dn_single), tc.dn_yard())
    if dn_pad == 0:
        b2, plain = _guarded(R, 256)
        ops.self_attn(qkv, out=plain, R=R, impl=impl)
        torch.cuda.synchronize()
        assert _intact(b2, R * 256) and _same_bits(out, plain)
        _hold('self_attn_dn', f'ops.self_attn impl={impl} R={R}', 'ctx', plain, tc.dn_refs(R, 0, 1), tc.dn_yard())


# ------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize('M', tc.LN_M)
def test_layer_norm_backward_rows(M):
    """mv2d_layer_norm_bwd: dx of every row (rows 0 and M - 1 constant: variance 0), dw and db per element; M = 0 gives dw = db = 0; the autograd
    node (M >= 1) returns the same bits and its forward holds too."""
    from mv2d_amd.autograd_ops import layer_norm
    lib = _lib()
    c = tc.ln_case(M)
    x, dy = (torch.cat([t, torch.zeros(1, 256)]).to(DEV) for t in (c.x, c.dy))          # (one row behind: a non-null pointer at M = 0)
    w, b = c.w.to(DEV), c.b.to(DEV)
    nb = int(lib.mv2d_layer_norm_bwd_blocks(M))
    assert nb == (M + 63) // 64
    (xb, dx), (wb, dw), (bb, db), (p0b, p0), (p1b, p1) = _guarded(M, 256), _guarded(1, 256), _guarded(1, 256), _guarded(nb, 256), _guarded(nb, 256)
    _check(lib.mv2d_layer_norm_bwd(_p(x), _p(dy), _p(w), _p(dx), _p(p0), _p(p1), _p(dw), _p(db), M, tc.LN_EPS, _st()), 'mv2d_layer_norm_bwd')
    torch.cuda.synchronize()
    assert _intact(xb, M * 256) and _intact(wb, 256) and _intact(bb, 256) and _intact(p0b, nb * 256) and _intact(p1b, nb * 256)
    ref = tc.ln_refs(M)
    if M == 0:
        assert float(dw.abs().max()) == 0.0 and float(db.abs().max()) == 0.0
        return
    _hold('ln_bwd', f'M={M}', 'dx', dx, ref.dx, tc.ln_yard('dx'))
    _hold('ln_bwd', f'M={M}', 'dw', dw[0], ref.dw, tc.ln_yard('dw'), vec=True)
    _hold('ln_bwd', f'M={M}', 'db', db[0], ref.db, tc.ln_yard('db'), vec=True)
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x[:M], w, b))
    y = layer_norm(xa, wa, ba, tc.LN_EPS)
    y.backward(dy[:M])
    assert _same_bits(xa.grad, dx) and _same_bits(wa.grad, dw[0]) and _same_bits(ba.grad, db[0])
    _hold('ln_bwd', f'M={M}', 'y', y.detach(), ref.y, tc.ln_yard('y'))


@pytest.mark.parametrize('cols', tc.CS_COLS)
@pytest.mark.parametrize('rows', tc.CS_ROWS)
def test_column_sums(rows, cols):
    """mv2d_colsum / mv2d_colsum_add per element against fp64 at ld = cols and cols + 3, with and without the scratch of the two-pass form (used
    above 1024 rows), plain, added to a separate vector and accumulated into `out`; rows = 0 gives 0, or `add` exactly."""
    lib = _lib()
    pool, add_all = tc.cs_pool()
    add = add_all[:cols].to(DEV)
    nch = int(lib.mv2d_colsum_scratch_rows(rows))
    assert nch == (0 if rows <= 1024 else (rows + 511) // 512)
    for ld in (cols, cols + tc.CS_PAD):
        x = torch.cat([pool[:rows, :ld], torch.zeros(1, ld)]).contiguous().to(DEV)
        for with_scratch in (False, True):
            for mode in ('plain', 'add', 'alias'):
                (ob, out), (sb, scratch) = _guarded(1, cols), _guarded(max(nch, 1), cols)
                if mode == 'alias':
                    out.copy_(add[None])
                sp = _p(scratch) if with_scratch else None
                if mode == 'plain':
                    _check(lib.mv2d_colsum(_p(x), ld, rows, cols, _p(out), sp, _st()), 'mv2d_colsum')
                else:
                    _check(lib.mv2d_colsum_add(_p(x), ld, rows, cols, _p(out), sp, _p(add if mode == 'add' else out), _st()), 'mv2d_colsum_add')
                torch.cuda.synchronize()
                tag = f'rows={rows} cols={cols} ld={ld} scratch={int(with_scratch)} {mode}'
                assert _intact(ob, cols) and _intact(sb, (nch if with_scratch else 0) * cols), tag
                want = tc.colsum(rows, cols, add=mode != 'plain')
                if rows == 0:
                    assert torch.equal(out[0].cpu().double(), want), tag
                else:
                    _hold('colsum', tag, 'sum', out[0], want, tc.cs_yard(), vec=True)


@pytest.mark.parametrize('dropped', [False, True])
@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('cols', tc.SM_COLS)
def test_softmax_backward_rows(cols, padded, dropped):
    """mv2d_softmax_bwd_rows in place: dS of every row against fp64 with Pd is P and with a dropped copy; the sentinel of the pad columns
    (ld = cols + 5) survives; one column gives exactly 0."""
    lib = _lib()
    c = tc.sm_case(cols, padded, dropped)
    P, Pd = c.P.to(DEV), c.Pd.to(DEV)
    buf, dP = _guarded(tc.SM_ROWS, c.ld)
    dP.copy_(c.dP)
    _check(lib.mv2d_softmax_bwd_rows(_p(P), _p(Pd if dropped else P), _p(dP), c.ld, tc.SM_ROWS, cols, float(c.keep_scale), _st()), 'mv2d_softmax_bwd_rows')
    torch.cuda.synchronize()
    assert _intact(buf, tc.SM_ROWS * c.ld) and bool((dP[:, cols:] == SENTINEL).all())
    want = tc.softmax_bwd(cols, padded, dropped)
    if cols == 1:
        assert float(dP[:, :1].abs().max()) == 0.0
    _hold('softmax_bwd', f'cols={cols} ld={c.ld} dropped={int(dropped)}', 'dS', dP[:, :cols], want, tc.sm_yard())
