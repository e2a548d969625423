"""The cross-attention kernels WITH lo rows against fp64, row by row, at the edges of the 16-key tile (-m gpu): csrc/xattn_walk.h through
ops.xattn_tile (1, 2, 4, 8 waves per query) and ops.xattn_fused, ops.xattn_ctxmap behind them, and the separate walk of csrc/xattn_group.hip.
The cases and the references are tests/xattn_cases.py; tests/test_xattn_cases_cpu.py shows that on the shared-hi rows a dropped, misplaced or
misscaled lo term moves a row by >= 0.5 (>= 64 yardsticks), where the yardstick is the largest per-row error of a plain fp32 evaluation of the
same operands (torch, CPU) against fp64.

The bound: per row, error <= K x yardstick with K = 8.  The kernels drop the lo x lo products and add three fp32-accumulated MFMAs per
product, so a small multiple of one fp32 evaluation is what to expect; measured on an MI355X (profiles/xattn_lo_rows_vs_fp64.txt) the largest
ratio over all kernels, formats, wave counts and cases is 2.48 (ctx of the random rows with key16 lo rows; 2.25 for z and 0.86 for the logits
of the tile kernel, 2.09 for the group kernel), and K is twice that, rounded up to a power of two.  K may never exceed 64, the room the CPU
test shows; a ratio beyond it is a finding about the kernel, not a reason to raise K.

Formats: 'key16' = hi + key16 lo rows, 'lo8' = hi + e4m3 lo rows (reference on the decoded bytes), 'hi' = hi rows alone.  What the launcher does
with `waves` (csrc/xattn_tile.hip): hi rows alone run 1, 2, 4 or 8 waves as asked; with lo rows 8 waves run as 2, and a launch that writes
dbg_logits runs 4 waves -- so with lo rows "z is bit for bit the same with and without dbg_logits" holds, and is asserted, at waves = 4; at the
other wave counts the z of the debug launch is held against fp64 like every other."""
import functools

import pytest
import torch

import xattn_cases as xc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -12345.0
K = 8.0
KINDS = {'hi0': lambda: xc.shared_hi_case(0, 2100), 'hi6': lambda: xc.shared_hi_case(6, 2106), 'random': lambda: xc.random_case(2200)}
FMTS = ('key16', 'lo8', 'hi')
# the global bounds of tests/test_gpu_kernels.py::test_xattn_tile_equals_projected_attention, unchanged, for the random rows
TOL_LOGITS, TOL_Z, TOL_CTX = 2e-5, 3e-5, 5e-5


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _guarded(shape, guard=4096):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + guard,), SENTINEL, device=DEV)
    return buf, buf[:n].view(shape)


def _intact(buf, n):
    return bool((buf[n:] == SENTINEL).all())


def _unpack_qt(Qt, R):
    """Qt [R,4096] key16 -> hi + lo [R,8,256] fp64: Qt[r][h][s][g][part][e] = part (hi | lo) of head h, channel 32 s + 8 g + e"""
    t = Qt.view(R, 8, 8, 4, 2, 8).double().cpu()
    return (t[:, :, :, :, 0] + t[:, :, :, :, 1]).reshape(R, 8, 256)


@functools.lru_cache(maxsize=None)
def _case(kind):
    from mv2d_amd import _lib, ops
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    _lib.load()
    if ops.key16_dtype() != torch.float16:
        pytest.skip('lo8 rows and the shared-hi construction need the fp16 key format')
    case = KINDS[kind]()
    d = lambda t: t.to(DEV)
    case.dev = dict(q=d(case.q), row_ptr=d(case.row_ptr), col=d(case.col_idx), bv=d(case.bv))
    khi, klo = ops.f32_to_key16(d(case.xk32), with_lo=True)
    vhi, vlo = ops.f32_to_key16(d(case.xv32), with_lo=True)
    for got, want in zip((khi, klo, vhi, vlo), xc.split_key16(case.xk32) + xc.split_key16(case.xv32)):      # the project's split == its restatement
        assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
    k8, v8 = ops.lo8_encode(klo), ops.lo8_encode(vlo)
    assert torch.equal(k8.cpu(), xc.lo8_encode(klo.cpu())) and torch.equal(ops.lo8_decode(k8).cpu().view(torch.int16), xc.lo8_decode(k8.cpu()).view(torch.int16))
    case.dev.update(khi=khi, vhi=vhi, lo={'key16': (klo, vlo), 'lo8': (k8, v8), 'hi': (None, None)})
    case.WA, case.WB = ops.pack_xattn_maps(d(case.Wk), d(case.Wv))
    case.dev['Qt'] = ops.xattn_qmap(case.dev['q'], case.WA)
    case.Qt64 = _unpack_qt(case.dev['Qt'], case.R)                    # the query map's own rounding is not charged to the walk ...
    qk = xc.qk_map(case.q, case.Wk)
    assert float((case.Qt64 - qk).abs().max() / qk.abs().max()) < 3e-5          # ... it has its bound here (test_xattn_tile_equals_projected_attention's)
    case.order = torch.roll(torch.arange(case.R - 1, -1, -1, dtype=torch.int32), 5).to(DEV)         # one fixed permutation, not the identity
    return case


@functools.lru_cache(maxsize=None)
def _refs(kind, fmt):
    """(case, fp64 reference, yardsticks, bases) on the operands the kernel decodes; shared by every test of the (case, format)"""
    case = _case(kind)
    klo, vlo = (t.cpu() if t is not None else None for t in case.dev['lo'][fmt])
    if fmt == 'lo8':
        klo, vlo = xc.lo8_decode(klo), xc.lo8_decode(vlo)
    ops_ = (case.dev['khi'].cpu(), klo, case.dev['vhi'].cpu(), vlo)
    ref = xc.attend(case, case.Qt64, *ops_)
    f32 = xc.attend(case, case.Qt64, *ops_, dtype=torch.float32)
    flat = case.kind == 'shared_hi' and fmt == 'hi'                   # every key of a row alike: nothing to take a row error of
    zb, cb = xc.bases(case, lo_free=fmt == 'hi')
    yard = None
    if not flat:
        many, has = case.nk >= 2, case.nk >= 1
        yard = dict(logits=float(xc.logit_row_errors(case, f32.logits, ref.logits, case.kind == 'shared_hi')[many if case.kind == 'shared_hi' else has].max()),
                    z=float(xc.row_errors(f32.z, ref.z, zb)[has].max()), ctx=float(xc.row_errors(f32.ctx, ref.ctx, cb)[has].max()))
    return case, ref, yard, (zb, cb), ops_


def _hold(tag, what, err, rows, yard):
    """per-row errors of the rows `rows` against K x the yardstick; prints the ratio"""
    worst = float(err[rows].max())
    at = int(err.nan_to_num(-1.0).masked_fill(~rows, -1.0).argmax())
    print(f'xattn_lo_ratio {tag} {what}: largest row error {worst:.3e} (row {at}) = {worst / yard[what]:.2f} x the fp32 evaluation ({yard[what]:.3e})')
    assert worst <= K * yard[what], (tag, what, worst / yard[what], err)


def _single_key_row(case, z, ops_):
    """the row with one key: z == that key's value row to fp32 rounding (p = 1; one rounding of hi + lo, one of the normalisation and its reciprocal)"""
    r = case.nk.tolist().index(1)
    key = int(case.col_idx[int(case.row_ptr[r])])
    v = ops_[2][key].double() + (ops_[3][key].double() if ops_[3] is not None else 0.0)
    assert float((z[r].double().cpu() - v).abs().max()) <= 2.0 ** -22 * float(v.abs().max())


@pytest.mark.parametrize('waves', [1, 2, 4, 8])
@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('kind', list(KINDS))
def test_xattn_tile_rows_against_fp64(kind, fmt, waves):
    """ops.xattn_tile: dbg_logits and z of every row against fp64 (the bound and the cases: the module docstring).  Largest measured ratio: see K."""
    from mv2d_amd import ops
    case, ref, yard, (zb, cb), ops_ = _refs(kind, fmt)
    dv = case.dev
    klo, vlo = dv['lo'][fmt]
    R, has, many = case.R, case.nk >= 1, case.nk >= 2
    empty = int(case.nk.tolist().index(0))
    run = lambda out, **kw: ops.xattn_tile(dv['Qt'], dv['khi'], dv['vhi'], dv['row_ptr'], dv['col'], out=out, waves=waves, Xk_lo=klo, Xv_lo=vlo, **kw)
    bufs = [_guarded((R, 8, 256)) for _ in range(4)]
    dbuf, dbg = _guarded((8, case.nnz))
    z_dbg = run(bufs[0][1], empty_nan=False, dbg_logits=dbg)
    z = run(bufs[1][1], empty_nan=False)
    z_ord = run(bufs[2][1], empty_nan=False, order=case.order)
    z_nan = run(bufs[3][1], empty_nan=True)
    torch.cuda.synchronize()
    assert all(_intact(b, R * 8 * 256) for b, _ in bufs) and _intact(dbuf, 8 * case.nnz)
    assert bool((dbg != SENTINEL).all()) and bool(torch.isfinite(dbg).all())                      # a logit for every listed pair
    # ---- structure
    assert torch.equal(z_ord.view(torch.int32), z.view(torch.int32))                            # any launch order: the same rows bit for bit
    if fmt == 'hi' or waves == 4:
        assert torch.equal(z_dbg.view(torch.int32), z.view(torch.int32))                        # the debug output only adds a store
    assert float(z[empty].abs().max()) == 0.0 and bool(torch.isnan(z_nan[empty]).all())            # the empty row, both policies
    keep = torch.arange(R) != empty
    assert torch.equal(z_nan[keep.to(DEV)].view(torch.int32), z[keep.to(DEV)].view(torch.int32))
    # ---- against fp64
    tag = f'tile kind={kind} fmt={fmt} waves={waves}'
    _single_key_row(case, z, ops_)
    if yard is None:
        rp = case.row_ptr.tolist()
        for r in range(R):                                                                      # identical operands, the same arithmetic order per column
            if rp[r + 1] > rp[r]:
                assert torch.equal(dbg[:, rp[r]:rp[r + 1]], dbg[:, rp[r]:rp[r] + 1].expand(-1, rp[r + 1] - rp[r])), r
        hv = case.hv[:, None, :].expand(-1, 8, -1)
        assert relerr(z[has.to(DEV)], hv[has]) < TOL_Z and relerr(z_dbg[has.to(DEV)], hv[has]) < TOL_Z
        return
    centre = case.kind == 'shared_hi'
    _hold(tag, 'logits', xc.logit_row_errors(case, dbg, ref.logits, centre), many if centre else has, yard)
    _hold(tag, 'z', xc.row_errors(z, ref.z, zb), has, yard)
    _hold(tag + ' (debug launch)', 'z', xc.row_errors(z_dbg, ref.z, zb), has, yard)
    if case.kind == 'random':
        assert relerr(dbg, ref.logits) < TOL_LOGITS and relerr(z, ref.z) < TOL_Z and relerr(z_dbg, ref.z) < TOL_Z


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('kind', list(KINDS))
def test_xattn_ctxmap_and_fused_rows_against_fp64(kind, fmt):
    """ops.xattn_ctxmap on the tile kernel's z and ops.xattn_fused (with and without a launch order): ctx of every row against fp64; the fused kernel
    is the three launches with one wave per query bit for bit; the empty row under both policies."""
    from mv2d_amd import ops
    case, ref, yard, (zb, cb), ops_ = _refs(kind, fmt)
    dv = case.dev
    klo, vlo = dv['lo'][fmt]
    R, has = case.R, case.nk >= 1
    empty = int(case.nk.tolist().index(0))
    res = {}
    for empty_nan in (False, True):
        z = ops.xattn_tile(dv['Qt'], dv['khi'], dv['vhi'], dv['row_ptr'], dv['col'], empty_nan=empty_nan, waves=1, Xk_lo=klo, Xv_lo=vlo)
        bufs = [_guarded((R, 256)) for _ in range(3)]
        ctx = ops.xattn_ctxmap(z, case.WB, dv['bv'], dv['row_ptr'], out=bufs[0][1], empty_nan=empty_nan)
        fused = ops.xattn_fused(dv['q'], case.WA, case.WB, dv['bv'], dv['khi'], dv['vhi'], dv['row_ptr'], dv['col'], out=bufs[1][1], empty_nan=empty_nan,
                                Xk_lo=klo, Xv_lo=vlo)
        fused_o = ops.xattn_fused(dv['q'], case.WA, case.WB, dv['bv'], dv['khi'], dv['vhi'], dv['row_ptr'], dv['col'], out=bufs[2][1], empty_nan=empty_nan,
                                  Xk_lo=klo, Xv_lo=vlo, order=case.order)
        torch.cuda.synchronize()
        assert all(_intact(b, R * 256) for b, _ in bufs)
        assert torch.equal(fused.view(torch.int32), ctx.view(torch.int32)) and torch.equal(fused_o.view(torch.int32), ctx.view(torch.int32))
        assert bool(torch.isnan(ctx[empty]).all()) if empty_nan else float(ctx[empty].abs().max()) == 0.0
        res[empty_nan] = ctx
    keep = (torch.arange(R) != empty).to(DEV)
    assert torch.equal(res[True][keep].view(torch.int32), res[False][keep].view(torch.int32))
    ctx = res[False]
    if yard is None:                                                  # hi rows alone, all keys of a row alike: ctx = Wv h_v + bv
        want = case.hv.double() @ case.Wv.double().T + case.bv.double()
        assert relerr(ctx[has.to(DEV)], want[has]) < TOL_CTX
        return
    _hold(f'ctxmap+fused kind={kind} fmt={fmt}', 'ctx', xc.row_errors(ctx, ref.ctx, cb), has, yard)
    if case.kind == 'random':
        assert relerr(ctx[has.to(DEV)], ref.ctx[has]) < TOL_CTX


@pytest.mark.parametrize('ordered', [False, True])
@pytest.mark.parametrize('kind', list(KINDS))
def test_xattn_group_rows_against_fp64(kind, ordered):
    """ops.xattn_group (csrc/xattn_group.hip: its own walk over the union of the key lists of 8 queries; key16 lo rows, it reads no e4m3 rows):
    ctx of every row against fp64 under the bound of the per-query kernels; tables as in test_xattn_group_tables_and_attention."""
    from mv2d_amd import ops
    case, ref, yard, (zb, cb), ops_ = _refs(kind, 'key16')
    dv = case.dev
    klo, vlo = dv['lo']['key16']
    R, has = case.R, case.nk >= 1
    empty = int(case.nk.tolist().index(0))
    order = case.order if ordered else None
    grp = torch.tensor([0, R], dtype=torch.int32, device=DEV)
    tab = ops.xattn_group_alloc(R, 1, case.nnz, DEV)
    ops.xattn_group_tables(dv['row_ptr'], dv['col'], grp, R, tab, order=order)
    assert int(tab['ctl'][1]) == 0
    res = {}
    for empty_nan in (False, True):
        buf, out = _guarded((R, 256))
        ops.xattn_group(dv['q'], case.WA, case.WB, dv['bv'], dv['khi'], dv['vhi'], dv['row_ptr'], tab, out=out, empty_nan=empty_nan, Xk_lo=klo, Xv_lo=vlo, order=order)
        torch.cuda.synchronize()
        assert _intact(buf, R * 256)
        assert bool(torch.isnan(out[empty]).all()) if empty_nan else float(out[empty].abs().max()) == 0.0
        res[empty_nan] = out
    keep = (torch.arange(R) != empty).to(DEV)
    assert torch.equal(res[True][keep].view(torch.int32), res[False][keep].view(torch.int32))
    _hold(f'group kind={kind} ordered={int(ordered)}', 'ctx', xc.row_errors(res[False], ref.ctx, cb), has, yard)
    if case.kind == 'random':
        assert relerr(res[False][has.to(DEV)], ref.ctx[has]) < TOL_CTX


def test_roi_align_lo8_rows_of_a_shared_hi_map():
    """The producer side, once: RoIAlign of a map whose pixels are one fp16 row h plus remainders below half an ulp writes e4m3 lo rows that are
    lo8_encode of its key16 lo rows, and does not raise the saturation flag (tests/test_gpu_kernels.py::test_lo8_row_format has the rest)."""
    from mv2d_amd import ops
    _case('hi0')
    H, W, R = 12, 20, 9
    g = torch.Generator().manual_seed(78)
    h = torch.randint(1025, 2048, (256,), generator=g).float() * 2.0 ** -10 * (torch.randint(0, 2, (256,), generator=g).float() * 2 - 1)
    m0 = (h.double() + (torch.rand((2 * H * W, 256), generator=g, dtype=torch.float64) * 0.4 + 0.05) * 2.0 ** -10
          * (torch.randint(0, 2, (2 * H * W, 256), generator=g).double() * 2 - 1)).float().to(DEV)
    x1, y1 = torch.rand(R, generator=g) * (W * 16 - 140), torch.rand(R, generator=g) * (H * 16 - 140)
    rois = torch.stack([torch.randint(0, 2, (R,), generator=g).float(), x1, y1, x1 + 8 + torch.rand(R, generator=g) * 120, y1 + 8 + torch.rand(R, generator=g) * 120], 1).to(DEV)
    hi, lo = (torch.zeros((R, 49, 256), device=DEV, dtype=torch.float16) for _ in range(2))
    b8 = torch.zeros((R, 49, 256), device=DEV, dtype=torch.uint8)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.roi_align(m0, rois, H, W, out0=hi, out0_lo=lo, out0_lo8=b8, lo8_flag=flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert torch.equal(b8, ops.lo8_encode(lo)) and float(lo.float().abs().max()) > 0.0
