"""The row side of a decoder layer at the edges of its block shapes (-m gpu): the row-block kernels of csrc/rowblock.hip through
ops.attn_out_fused_x3, ops.attn_out_qmap_x3, ops.attn_out_zmap_x3 and ops.ffn_out_fused_x3, and the self-attention core (csrc/self_attn_x3.hip,
and csrc/attention.hip as impl='f32') through ops.self_attn.  Cases, references and the format model: tests/rowblock_cases.py;
tests/test_rowblock_cases_cpu.py shows that one lost lo product moves every row by >= 3 x K_ROWS yardsticks and one mishandled last key by
>= 4 x K_SA, where a yardstick is the largest per-row error of a plain fp32 evaluation (torch, CPU) of the same operands against fp64.

Which launch reaches which kernel instance (the launchers take 16 rows per block, RT = 1, up to M = 512 and 32 rows per block, RT = 2, above):
    M = 1, 16, 17, 512      attn_out_fused_x3_kernel<1, false, false> (attn_out_fused_x3), <1, false, true> (attn_out_qmap_x3),
                            <1, true, false> (attn_out_zmap_x3), ffn_out_fused_x3_kernel<1>; and every [0:512] / [512:M] launch of the
                            block-shape identities
    M = 513, 528, 529, 545  attn_out_fused_x3_kernel<2, false, false>, <2, false, true>, <2, true, false>, ffn_out_fused_x3_kernel<2>:
                            one row in the last block, its second tile empty, one row in its second tile, 17 full blocks plus one row
Every output lies in front of a guard region of 32 rows filled with a sentinel that must be intact after every launch.

Bit for bit (no tolerance; NaN rows: NaN in the same places, equal elsewhere): attn_out_qmap_x3 == attn_out_fused_x3 (q stage on) followed by
xattn_qmap; attn_out_zmap_x3 == xattn_ctxmap followed by attn_out_fused_x3, with empty_nan on and off; one RT = 2 launch == two RT = 1
launches over [0:512] and [512:M] for all four entries and every combination of the optional outputs of the FFN tail; the FFN tail's x, xq
and outs == ops.row_ln's at every M and 1, 4, 7, 23, 32 slabs; every sample of a batched self-attention launch == its single-sample launch
(both impls, a tight and a loose max_grp_rows), the padding rows untouched.

Per row against fp64: error <= K x yardstick for every output of every entry at every M.  Measured on an MI355X (fp16-pair build; the lines
of -s are profiles/rowblock_rows_vs_fp64.txt), largest ratio per family and K = twice that, rounded up to a power of two:
    row kernels             1.40 (Qt of attn_out_qmap_x3 and xattn_qmap; x 1.07, q 0.94, z-form x 1.12, y 1.14, xq 1.28, outs 1.02,
                            qkv 1.00: the worst rows lie in front of row 512, so every M >= 512 shows them)          K_ROWS = 4
    self-attention x3 plain 0.69                                                                              K_SA_X3_PLAIN = 2
    self-attention x3 sharp 0.60                                                                              K_SA_X3_SHARP = 2
    self-attention f32      0.89 (plain; 0.74 sharp)                                                               K_SA_F32 = 2
What the bounds and identities were seen to catch, each in a scratch build of the library: the q_out store of attn_out_fused_x3_kernel without its
`m < p.M` guard (guard regions overwritten at M = 1, 17, 513, 528, 529, 545), the a_lo w_hi MFMA of tile_mma_x3 dropped (x of every entry at
316 .. 772 yardsticks), the padding keys of the last 32-key step of self_attn_x3_kernel unmasked (8e5 and 4e6 yardsticks).
The caps K_ROWS <= 16 and K_SA <= 64 (rowblock_cases.py) are what the CPU test justifies; a ratio beyond them is a finding about the kernel,
not a reason to raise K.  The bounds are those of the shipped fp16-pair format: a bf16 build (mv2d_q16_format() != 1) runs the identities and
skips the comparison with fp64."""
import functools

import pytest
import torch

import rowblock_cases as rc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -12345.0
GUARD_ROWS = 32
F64, F32 = torch.float64, torch.float32
BIG = [M for M in rc.ROW_COUNTS if M > 512]
SA_MAX = max(rc.SA_SIZES)


# ------------------------------------------------------------------------------------------------ helpers
def _guarded(rows, width, dtype=torch.float32, live=None):
    """(buffer, view [rows, width]): `live` (default `rows`) rows for the launch, the rest of the view and GUARD_ROWS rows behind it sentinel"""
    buf = torch.full(((rows + GUARD_ROWS) * width,), SENTINEL, device=DEV, dtype=dtype)
    return buf, buf[:rows * width].view(rows, width)


def _intact(buf, n):
    return bool((buf[n:] == buf.new_tensor(SENTINEL)).all())


def _same_bits(a, b):
    """NaN in the same places, the same bits elsewhere"""
    na, nb = torch.isnan(a), torch.isnan(b)
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a.masked_fill(na, 0.0).view(it), b.masked_fill(nb, 0.0).view(it))


def _unpack_qt(Qt, R):
    """Qt [R,4096] key16 -> hi + lo [R,8,256] fp64: Qt[r][h][s][g][part][e] = part (hi | lo) of head h, channel 32 s + 8 g + e"""
    t = Qt.view(R, 8, 8, 4, 2, 8).double().cpu()
    return (t[:, :, :, :, 0] + t[:, :, :, :, 1]).reshape(R, 8, 256)


@functools.lru_cache(maxsize=None)
def _dev():
    """operands on the device once per module, weights packed once"""
    from mv2d_amd import _lib, ops
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    _lib.load()
    o = rc.operands()
    d = type(o)(**{k: v.to(DEV) for k, v in vars(o).items()})
    d.Wo_x3, d.Wq_x3, d.Win_x3 = ops.pack_x3(d.Wo), ops.pack_x3(d.Wq), ops.pack_x3(d.Win)
    d.WA, d.WB = ops.pack_xattn_maps(d.Wk, d.Wv)
    d.fp16 = ops.q16_dtype() == torch.float16 and ops.key16_dtype() == torch.float16
    d.qt_dtype = ops.key16_dtype()
    return d


@functools.lru_cache(maxsize=None)
def _yard(name, n_parts=rc.N_PARTS_ALL):
    """the yardstick of an output: over all 545 rows (the z-form x: over those with a key), as in tests/test_rowblock_cases_cpu.py"""
    if name in ('x', 'q', 'Qt'):
        return rc.yardstick(getattr(rc.attn_refs(F32), name), getattr(rc.attn_refs(F64), name))
    if name == 'zx':
        return rc.yardstick(rc.zmap_refs(F32, False).x, rc.zmap_refs(F64, False).x, ~rc.operands().empty)
    return rc.yardstick(getattr(rc.tail_refs(F32, n_parts), name), getattr(rc.tail_refs(F64, n_parts), name))


def _hold(tag, what, got, want, yard, K, rows=None):
    """per-row errors of `got` (rows `rows`, default all) against K x the yardstick; prints the ratio in one line"""
    if not _dev().fp16:
        return
    err = rc.row_errors(got, want)
    if rows is not None:
        err = err.masked_fill(~rows, 0.0)
    worst, at = float(err.max()), int(err.nan_to_num(float('inf')).argmax())
    print(f'rowblock_ratio {tag} {what}: largest row error {worst:.3e} (row {at}) = {worst / yard:.2f} x the fp32 evaluation ({yard:.3e})')
    assert worst <= K * yard, (tag, what, worst / yard)               # (a NaN fails the comparison)


def _skip_fp64_on_bf16():
    if not _dev().fp16:
        pytest.skip('identities hold; the fp64 bounds are those of the fp16-pair format')


# ------------------------------------------------------------------------------------------------ the entries on rows [a:b]
def _attn(a, b, q_stage):
    from mv2d_amd import ops
    d, M = _dev(), b - a
    xb, x = _guarded(M, 256)
    qb, q = _guarded(M, 256)
    kw = dict(qpos=d.qpos[a:b], Wq_x3=d.Wq_x3, bq=d.bq, qscale=rc.QSCALE, q_out=q) if q_stage else {}
    ops.attn_out_fused_x3(d.ctx[a:b], d.resid[a:b], d.Wo_x3, d.bo, (d.lw, d.lb), x, M=M, **kw)
    torch.cuda.synchronize()
    assert _intact(xb, M * 256) and _intact(qb, M * 256 if q_stage else 0), ('attn_out_fused_x3', a, b, q_stage)
    return x, (q if q_stage else None)


def _qmap(a, b):
    from mv2d_amd import ops
    d, M = _dev(), b - a
    xb, x = _guarded(M, 256)
    tb, Qt = _guarded(M, 4096, d.qt_dtype)
    ops.attn_out_qmap_x3(d.ctx[a:b], d.resid[a:b], d.Wo_x3, d.bo, (d.lw, d.lb), x, qpos=d.qpos[a:b], Wq_x3=d.Wq_x3, bq=d.bq, qscale=rc.QSCALE,
                         WA=d.WA, Qt=Qt, M=M)
    torch.cuda.synchronize()
    assert _intact(xb, M * 256) and _intact(tb, M * 4096), ('attn_out_qmap_x3', a, b)
    return x, Qt


def _zmap(a, b, empty_nan):
    from mv2d_amd import ops
    d, M = _dev(), b - a
    xb, x = _guarded(M, 256)
    ops.attn_out_zmap_x3(d.z[a:b], d.WB, d.bv, d.row_ptr[a:], d.resid[a:b], d.Wo_x3, d.bo, (d.lw, d.lb), x, empty_nan=empty_nan, M=M)
    torch.cuda.synchronize()
    assert _intact(xb, M * 256), ('attn_out_zmap_x3', a, b, empty_nan)
    return x


def _ffn(a, b, n_parts, in_proj=True, outs=True, xq=True):
    from mv2d_amd import ops
    d, M = _dev(), b - a
    bufs = {k: _guarded(M, w) for k, w in (('x', 256), ('xq', 256), ('outs', 256), ('qkv', 768))}
    on = dict(x=True, xq=xq, outs=outs, qkv=in_proj)
    v = {k: bufs[k][1] if on[k] else None for k in bufs}
    kw = dict(Win_x3=d.Win_x3, b_in=d.b_in, qkv=v['qkv']) if in_proj else {}
    ops.ffn_out_fused_x3(d.parts[:n_parts, a:b], d.b2, d.resid[a:b], (d.tw, d.tb), (d.pw, d.pb) if outs else None, v['x'], d.qpos[a:b], v['xq'],
                         outs=v['outs'], M=M, **kw)
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert _intact(buf, view.numel() if on[k] else 0), ('ffn_out_fused_x3', k, a, b, n_parts, in_proj, outs, xq)
    return v


# ------------------------------------------------------------------------------------------------ out-projection rows
@pytest.mark.parametrize('M', rc.ROW_COUNTS)
def test_attn_out_and_qmap_rows(M):
    """attn_out_fused_x3 with and without the q stage and attn_out_qmap_x3 on the first M rows: the same x bit for bit, Qt bit for bit what
    xattn_qmap makes of that launch's q; x, q and Qt of every row against fp64."""
    from mv2d_amd import ops
    d = _dev()
    x, q = _attn(0, M, True)
    x_only, _ = _attn(0, M, False)
    xm, Qt = _qmap(0, M)
    rb, Qt_chain = _guarded(M, 4096, d.qt_dtype)
    ops.xattn_qmap(q, d.WA, Qt=Qt_chain, R=M)
    torch.cuda.synchronize()
    assert _intact(rb, M * 4096)
    assert _same_bits(x_only, x) and _same_bits(xm, x) and _same_bits(Qt, Qt_chain)
    ref = rc.attn_refs(F64)
    _hold(f'attn_out_fused_x3 M={M}', 'x', x, ref.x[:M], _yard('x'), rc.K_ROWS)
    _hold(f'attn_out_fused_x3 M={M}', 'q', q, ref.q[:M], _yard('q'), rc.K_ROWS)
    _hold(f'attn_out_qmap_x3 M={M}', 'x', xm, ref.x[:M], _yard('x'), rc.K_ROWS)
    _hold(f'attn_out_qmap_x3 M={M}', 'Qt', _unpack_qt(Qt, M), ref.Qt[:M], _yard('Qt'), rc.K_ROWS)
    _hold(f'xattn_qmap M={M}', 'Qt', _unpack_qt(Qt_chain, M), ref.Qt[:M], _yard('Qt'), rc.K_ROWS)
    _skip_fp64_on_bf16()


@pytest.mark.parametrize('empty_nan', [True, False])
@pytest.mark.parametrize('M', rc.ROW_COUNTS)
def test_attn_out_zmap_rows(M, empty_nan):
    """attn_out_zmap_x3 == xattn_ctxmap -> attn_out_fused_x3 bit for bit; the rows without a key (first and last row of a tile among them) are
    all-NaN and no other row is (empty_nan), or LN(bo + resid) (not LN(bv Wo^T + ...)); every row with a key against fp64."""
    from mv2d_amd import ops
    d = _dev()
    x = _zmap(0, M, empty_nan)
    cb, ctx = _guarded(M, 256)
    ops.xattn_ctxmap(d.z[:M], d.WB, d.bv, d.row_ptr, out=ctx, R=M, empty_nan=empty_nan)
    xb, x_chain = _guarded(M, 256)
    ops.attn_out_fused_x3(ctx, d.resid[:M], d.Wo_x3, d.bo, (d.lw, d.lb), x_chain, M=M)
    torch.cuda.synchronize()
    assert _intact(cb, M * 256) and _intact(xb, M * 256)
    assert _same_bits(x, x_chain)
    empty = rc.operands().empty[:M]
    nan_rows = torch.isnan(x).cpu()
    if empty_nan:
        assert torch.equal(nan_rows.all(1), empty) and torch.equal(nan_rows.any(1), empty)
    else:
        assert not bool(nan_rows.any())
    ref = rc.zmap_refs(F64, empty_nan).x[:M]
    if bool((~empty).any()):
        _hold(f'attn_out_zmap_x3 M={M} empty_nan={int(empty_nan)}', 'x', x, ref, _yard('zx'), rc.K_ROWS, rows=~empty)
    if not empty_nan:
        o = rc.operands()
        want = torch.nn.functional.layer_norm((o.bo.double() + o.resid.double())[:M], (256,), o.lw.double(), o.lb.double(), rc.EPS)
        _hold(f'attn_out_zmap_x3 M={M} empty_nan=0 (rows without a key)', 'x', x, want, _yard('zx'), rc.K_ROWS, rows=empty)
    _skip_fp64_on_bf16()


# ------------------------------------------------------------------------------------------------ FFN tail rows
@pytest.mark.parametrize('n_parts', rc.PARTS_COUNTS)
@pytest.mark.parametrize('M', rc.ROW_COUNTS)
def test_ffn_out_rows(M, n_parts):
    """ffn_out_fused_x3 on the first M rows and n_parts slabs: x, xq and outs are ops.row_ln's bit for bit, the last-layer form (no in-projection,
    no post-norm output) writes the same x and xq; y, xq, outs and qkv of every row against fp64."""
    from mv2d_amd import ops
    d = _dev()
    v = _ffn(0, M, n_parts)
    bufs = [_guarded(M, 256) for _ in range(3)]
    ops.row_ln(d.parts[:n_parts], bias=d.b2, residual=d.resid[:M], ln=(d.tw, d.tb), out=bufs[0][1], addvec=d.qpos[:M], out_plus=bufs[1][1],
               ln2=(d.pw, d.pb), out2=bufs[2][1], M=M)
    torch.cuda.synchronize()
    assert all(_intact(b, M * 256) for b, _ in bufs)
    assert _same_bits(v['x'], bufs[0][1]) and _same_bits(v['xq'], bufs[1][1]) and _same_bits(v['outs'], bufs[2][1])
    last = _ffn(0, M, n_parts, in_proj=False, outs=False)
    assert _same_bits(last['x'], v['x']) and _same_bits(last['xq'], v['xq'])
    ref = rc.tail_refs(F64, n_parts)
    for k, name in (('x', 'y'), ('xq', 'xq'), ('outs', 'outs'), ('qkv', 'qkv')):
        _hold(f'ffn_out_fused_x3 M={M} n_parts={n_parts}', name, v[k], getattr(ref, name)[:M], _yard(name, n_parts), rc.K_ROWS)
    _skip_fp64_on_bf16()


# ------------------------------------------------------------------------------------------------ both block shapes
def _cat(a, b):
    return torch.cat([a, b], 0)


@pytest.mark.parametrize('M', BIG)
def test_attn_out_block_shapes_agree(M):
    """One launch with 32 rows per block (M > 512) writes, row for row, what two launches with 16 rows per block over [0:512] and [512:M] write:
    attn_out_fused_x3 with and without the q stage, attn_out_qmap_x3, attn_out_zmap_x3 under both empty-row policies."""
    for q_stage in (True, False):
        x, q = _attn(0, M, q_stage)
        (x0, q0), (x1, q1) = _attn(0, 512, q_stage), _attn(512, M, q_stage)
        assert _same_bits(x, _cat(x0, x1)), q_stage
        assert not q_stage or _same_bits(q, _cat(q0, q1))
    x, Qt = _qmap(0, M)
    (x0, t0), (x1, t1) = _qmap(0, 512), _qmap(512, M)
    assert _same_bits(x, _cat(x0, x1)) and _same_bits(Qt, _cat(t0, t1))
    for empty_nan in (True, False):
        assert _same_bits(_zmap(0, M, empty_nan), _cat(_zmap(0, 512, empty_nan), _zmap(512, M, empty_nan))), empty_nan


@pytest.mark.parametrize('in_proj', [True, False])
@pytest.mark.parametrize('M', BIG)
def test_ffn_out_block_shapes_agree(M, in_proj):
    """The same for ffn_out_fused_x3 with and without the in-projection, with and without outs and xq_out (23 slabs: all three loops of the sum)."""
    for outs in (True, False):
        for xq in (True, False):
            one, lo, hi = (_ffn(a, b, 23, in_proj, outs, xq) for a, b in ((0, M), (0, 512), (512, M)))
            for k, full in one.items():
                assert (full is None) == (not dict(x=True, xq=xq, outs=outs, qkv=in_proj)[k])
                assert full is None or _same_bits(full, _cat(lo[k], hi[k])), (k, outs, xq)


# ------------------------------------------------------------------------------------------------ self-attention
@functools.lru_cache(maxsize=None)
def _sa_dev(kind):
    _dev()
    case = rc.sa_case(kind)
    return case, case.qkv.to(DEV), case.grp_start.to(DEV)


def _sa_batch(kind, impl, max_grp_rows):
    """the batched launch into a sentinel-filled buffer of R + SA_PAD rows with a guard behind: (ctx [R,256], after checking padding and guard)"""
    from mv2d_amd import ops
    case, qkv, grp = _sa_dev(kind)
    buf, ctx = _guarded(case.R + rc.SA_PAD, 256)
    ops.self_attn(qkv, out=ctx, R=case.R, grp_start=grp, max_grp_rows=max_grp_rows, impl=impl)
    torch.cuda.synchronize()
    assert _intact(buf, case.R * 256), (kind, impl, max_grp_rows)      # the 40 padding rows and the guard
    return ctx[:case.R]


@pytest.mark.parametrize('impl,max_grp_rows', [('x3', SA_MAX), ('x3', SA_MAX + 23), ('f32', 0)])
@pytest.mark.parametrize('kind', ['plain', 'sharp'])
def test_self_attn_batch_rows_equal_single_sample_launches(kind, impl, max_grp_rows):
    """Sample sizes on both sides of 16, 32, 64, 128 and 256: every sample's rows in the batched launch are bit for bit its single-sample
    launch's, with a tight and a loose per-sample row bound; the padding rows behind the batch are not written."""
    from mv2d_amd import ops
    case, qkv, _ = _sa_dev(kind)
    out = _sa_batch(kind, impl, max_grp_rows)
    for o, n in zip(case.starts, case.sizes):
        buf, single = _guarded(n, 256)
        ops.self_attn(qkv[o:o + n].contiguous(), out=single, R=n, impl=impl)
        torch.cuda.synchronize()
        assert _intact(buf, n * 256), (impl, n)
        assert _same_bits(out[o:o + n], single), (impl, n)


@pytest.mark.parametrize('impl', ['x3', 'f32'])
@pytest.mark.parametrize('kind', ['plain', 'sharp'])
def test_self_attn_rows_against_fp64(kind, impl):
    """ctx of every row of every sample against masked softmax attention in fp64; the one-key sample is its value row."""
    case, ref, yard = rc.sa_refs(kind)
    out = _sa_batch(kind, impl, SA_MAX if impl == 'x3' else 0)
    assert bool(torch.isfinite(out).all())
    v = case.qkv[0, 512:].double()
    assert float((out[0].double().cpu() - v).abs().max()) <= 2.0 ** -22 * float(v.abs().max())
    _skip_fp64_on_bf16()
    K = rc.K_SA_F32 if impl == 'f32' else (rc.K_SA_X3_PLAIN if kind == 'plain' else rc.K_SA_X3_SHARP)
    err = rc.row_errors(out, ref)
    for o, n in zip(case.starts, case.sizes):
        worst = float(err[o:o + n].max())
        print(f'rowblock_ratio self_attn impl={impl} kind={kind} sample of {n}: largest row error {worst:.3e} = {worst / yard:.2f} x the fp32 evaluation ({yard:.3e})')
    _hold(f'self_attn impl={impl} kind={kind}', 'ctx', out, ref, yard, K)
