"""The kernels that share one body since csrc/roiconv_walk.h against the bits of the spelled-out copies they replaced (-m gpu).

Until the runtime-size RoI conv walk lived in one header, tests/test_gpu_qg_shape.py's "the conv sums of a cell are bit for bit those the pooled
kernels add up" compared two separately written kernels; it now compares one body with itself.  The anchor here is older:
tests/golden/conv_walk_parent_bits.json holds, for every case below, the SHA-256 of the output bytes that the library of the commit BEFORE the
merge wrote, recorded on an MI355X with `digests` of this module (tests/golden/README_conv_walk_parent_bits.md).  The same goes for the two fp32
64 x 64 transpositions (csrc/rows.hip) and the 7 x 7 / s x s unfold pairs (csrc/train_ops.hip), which became wrappers of one body each.

Inputs come from seeds (rnd of tests/test_gpu_qg_shape.py, the conv operands of its _conv_operands); every output goes to a NaN-filled (masked
transposition: sentinel-filled) buffer one RoI / one row longer than what is written, and the tail has to stay.
  ops.qg_conv_cells, both precision forms, outputs hi / lo / fp32: R = 1, 3; s = 1 (one valid tap), 2 (all-border cells), 7 (the resident single
    chunk), 8 (exactly 64 cells), 9 (the first two-chunk size), 14 (four chunks with the moving window).
  ops.qg_conv_pool, ops.qg_conv_pool_x3: the same R and s (s = 7 goes through the 7 x 7 kernels and pins them too); the key16 entry also at
    R = 1025, s = 7: the smallest R that takes the two-RoIs-per-block instance with an odd tail.
  ops.nchw_to_nhwc, fp32, full and masked: V = 2, Cn = 68, HW = 76 (a ragged channel tile and a ragged position tile); the mask has one 64-position
    block all zero and the others partly set, and the rows of y whose byte is clear keep their sentinel.
  mv2d_im2col3x3(_s), mv2d_col2im3x3(_s): R = 3; s = 1, 7, 9, 14 (s = 7 through the entries without a size argument).

Nothing here goes through expf / logf: sums and products in a fixed order (-ffp-contract=off) and MFMAs, so a digest does not depend on the
toolchain's math library; the fixture still names the compiler that built the recorded library, and a failure prints it."""
import hashlib
import json
import os

import pytest
import torch

import test_gpu_qg_shape as qs
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV, NAN = qs.DEV, qs.NAN
SENTINEL = -7.0
RS, SS = (1, 3), (1, 2, 7, 8, 9, 14)
R_PAIRS = 1025
UNFOLD_R, UNFOLD_SS = 3, (1, 7, 9, 14)
V, CN, HW = 2, 68, 76
FIXTURE = os.path.join(GOLDEN, 'conv_walk_parent_bits.json')


def _digest(t):
    """what the fixture keeps of an output tensor"""
    a = t.detach().cpu().contiguous().view(-1)
    return {'sha256': hashlib.sha256(a.view(torch.uint8).numpy().tobytes()).hexdigest(), 'first8': [float(v) for v in a[:8]],
            'last8': [float(v) for v in a[-8:]]}


def _guarded(rows, shape, dtype, fill=NAN):
    """a filled buffer of rows + 1 leading entries"""
    return torch.full((rows + 1, *shape), fill, device=DEV, dtype=dtype)


def _written(buf, rows):
    """the first `rows` entries of a NaN-filled buffer, all written, and nothing behind them"""
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[rows:].float()).all()), 'a write past the output'
    assert bool(torch.isfinite(buf[:rows].float()).all()), 'an output element was not written'
    return _digest(buf[:rows])


def _cells_in(R, s):
    """(hi, lo) key16 cells [R, s*s, 256]; R_PAIRS RoIs are 41 seeded ones 25 times over"""
    from mv2d_amd import ops
    x = qs.rnd((min(R, 41), s * s, 256), 3100 + s)
    if R > 41:
        x = x.repeat(R // 41, 1, 1)
    return ops.f32_to_key16(x.to(DEV), with_lo=True)


def cells_digests(R, s):
    """{case id: digest} of the three outputs of ops.qg_conv_cells in both precision forms"""
    from mv2d_amd import ops
    op, k16, got = qs._conv_operands(), ops.key16_dtype(), {}
    hi, lo = _cells_in(R, s)
    for form, l, w in (('key16', None, op['wp']), ('x3', lo, op['wx3'])):
        oh, ol, of = (_guarded(R, (s * s, 256), dt) for dt in (k16, k16, torch.float32))
        ops.qg_conv_cells(hi, l, w, op['bd'], out_hi=oh, out_lo=ol, out_f32=of, R=R, roi_size=s)
        for name, t in (('hi', oh), ('lo', ol), ('f32', of)):
            got[f'qg_conv_cells/{form}/R{R}/s{s}/{name}'] = _written(t, R)
    return got


def pool_digests(R, s):
    """{case id: digest} of ops.qg_conv_pool and, below R_PAIRS, ops.qg_conv_pool_x3"""
    from mv2d_amd import ops
    op, got = qs._conv_operands(), {}
    hi, lo = _cells_in(R, s)
    out = _guarded(R, (256,), torch.float32)
    ops.qg_conv_pool(hi, op['wp'], op['bd'], out, R=R, roi_size=s)
    got[f'qg_conv_pool/R{R}/s{s}/out'] = _written(out, R)
    if R < R_PAIRS:
        out = _guarded(R, (256,), torch.float32)
        ops.qg_conv_pool_x3(hi, lo, op['wx3'], op['bd'], out, R=R, roi_size=s)
        got[f'qg_conv_pool_x3/R{R}/s{s}/out'] = _written(out, R)
    return got


def _mask():
    """uint8 [V * HW]: view 0 has its first 64-position block all zero and its ragged block partly set, view 1 both blocks partly set"""
    m = (torch.arange(V * HW) % 3 == 1).to(torch.uint8)
    m[:64] = 0
    assert m[64:HW].any() and not m[64:HW].all()
    return m


def transpose_digests(masked):
    """{case id: digest} of ops.nchw_to_nhwc on an fp32 map, full or masked"""
    from mv2d_amd import ops
    x = qs.rnd((V, CN, 4, HW // 4), 3200).to(DEV)
    if not masked:
        y = _guarded(V * HW, (CN,), torch.float32)
        ops.nchw_to_nhwc(x, out=y[:V * HW])
        return {'nchw_to_nhwc/full/y': _written(y, V * HW)}
    m = _mask()
    y = _guarded(V * HW, (CN,), torch.float32, SENTINEL)
    ops.nchw_to_nhwc(x, out=y[:V * HW], mask=m.to(DEV))
    torch.cuda.synchronize()
    rows = y[:V * HW].cpu()
    assert bool((y[V * HW:] == SENTINEL).all()), 'a write past the output'
    assert bool((rows[m == 0] == SENTINEL).all()), 'a row whose mask byte is clear was written'
    assert bool((rows[m == 1] != SENTINEL).all()), 'a listed row was not written'
    return {'nchw_to_nhwc/masked/y': _digest(y[:V * HW])}


def unfold_digests(s):
    """{case id: digest} of the unfold [R, s*s, 256] -> [R*s*s, 2304] and of its gradient, through the entries the autograd function takes"""
    from mv2d_amd import _lib
    from mv2d_amd.ops import _p, _stream, check
    lib, R, n = _lib.load(), UNFOLD_R, UNFOLD_R * s * s
    x, g = qs.rnd((R, s * s, 256), 3300 + s).to(DEV), qs.rnd((n, 2304), 3400 + s).to(DEV)
    cols, dx = _guarded(n, (2304,), torch.float32), _guarded(R, (s * s, 256), torch.float32)
    if s == 7:
        check(lib.mv2d_im2col3x3(_p(x), _p(cols), R, _stream()), 'mv2d_im2col3x3')
        check(lib.mv2d_col2im3x3(_p(g), _p(dx), R, _stream()), 'mv2d_col2im3x3')
    else:
        check(lib.mv2d_im2col3x3_s(_p(x), _p(cols), R, s, _stream()), 'mv2d_im2col3x3_s')
        check(lib.mv2d_col2im3x3_s(_p(g), _p(dx), R, s, _stream()), 'mv2d_col2im3x3_s')
    return {f'im2col3x3/R{R}/s{s}/cols': _written(cols, n), f'col2im3x3/R{R}/s{s}/dx': _written(dx, R)}


def digests():
    """every case of this module, as the fixture's "cases" (recording: README_conv_walk_parent_bits.md)"""
    got = {}
    for R in RS:
        for s in SS:
            got.update(cells_digests(R, s))
            got.update(pool_digests(R, s))
    got.update(pool_digests(R_PAIRS, 7))
    for masked in (False, True):
        got.update(transpose_digests(masked))
    for s in UNFOLD_SS:
        got.update(unfold_digests(s))
    return got


def _check(got):
    with open(FIXTURE) as fh:
        fixture = json.load(fh)
    want = fixture['cases']
    bad = [k for k in got if got[k]['sha256'] != want[k]['sha256']]
    for k in bad:
        print(f'[parent bits] {k}: recorded first8 {want[k]["first8"]} last8 {want[k]["last8"]}\n{"":14s}{"":{len(k)}s}  got      first8 '
              f'{got[k]["first8"]} last8 {got[k]["last8"]}')
    assert not bad, f'{len(bad)} of {len(got)} outputs differ from the recorded library (built with: {fixture["hipcc_version"]}): {bad}'


@pytest.mark.parametrize('s', SS)
@pytest.mark.parametrize('R', RS)
def test_conv_cells_write_the_parent_bits(R, s):
    _check(cells_digests(R, s))


@pytest.mark.parametrize('R,s', [(R, s) for R in RS for s in SS] + [(R_PAIRS, 7)])
def test_conv_pool_writes_the_parent_bits(R, s):
    _check(pool_digests(R, s))


@pytest.mark.parametrize('masked', [False, True], ids=['full', 'masked'])
def test_fp32_transposition_writes_the_parent_bits(masked):
    _check(transpose_digests(masked))


@pytest.mark.parametrize('s', UNFOLD_SS)
def test_unfold_pair_writes_the_parent_bits(s):
    _check(unfold_digests(s))


def test_fixture_lists_exactly_these_cases():
    with open(FIXTURE) as fh:
        fixture = json.load(fh)
    want = {f'qg_conv_cells/{f}/R{R}/s{s}/{o}' for f in ('key16', 'x3') for R in RS for s in SS for o in ('hi', 'lo', 'f32')}
    want |= {f'{e}/R{R}/s{s}/out' for e in ('qg_conv_pool', 'qg_conv_pool_x3') for R in RS for s in SS} | {f'qg_conv_pool/R{R_PAIRS}/s7/out'}
    want |= {'nchw_to_nhwc/full/y', 'nchw_to_nhwc/masked/y'}
    want |= {f'{e}/R{UNFOLD_R}/s{s}/{o}' for s in UNFOLD_SS for e, o in (('im2col3x3', 'cols'), ('col2im3x3', 'dx'))}
    assert set(fixture['cases']) == want and fixture['hipcc_version']
