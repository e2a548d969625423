"""The split-precision prediction branches (csrc/branches_x3.hip) against the bits of the kernels they replaced (-m gpu).

Until the four branch kernels became two, tests/test_gpu_branch_depth.py::test_depth_2_equals_the_shipped_launches compared two separately
written kernels; it now compares an instance with itself.  The anchor here is older: tests/golden/branches_parent_bits.json holds, for every
case below, the SHA-256 of the output bytes that the library of the commit BEFORE the merge wrote (heads_fused_x3_kernel, reg_layer_x3_kernel,
heads_depth_x3_kernel, reg_layer_depth_x3_kernel), recorded on an MI355X with `digests` of this module (tests/golden/
README_branches_parent_bits.md).  All seven C entries must still write exactly those bytes.

Inputs come from seeds: rows and reference points of tests/test_gpu_branch_depth.py::_rows, weights of its _tables (synthetic.make_head_state +
with_branch_depth_state); the tables of the first entries are packed from the depth-2 state, so at depth 2 both families of entries see the same
weights.  L = 2 (a wrong layer stride shows from the second layer on); M = 1 (one row), 17 (a partial second tile at one row tile per block), 77
(several blocks), 531 (two row tiles per block, ragged), 1100 (four row tiles per block, ragged, the last block with empty tiles); NC = 1, 10, 26,
64 (one masked class tile, the 10-class instance, two and four tiles); every group layout of tests/test_gpu_branch_depth.py.  Half the cases
divide the velocity by dt_rows with zeros in it, the other half by the scalar dt = 0.5.  Outputs go to guarded buffers.

A digest depends on the toolchain's expf / logf in the columns 0, 1 and 4 of a box code: the fixture names the compiler that built the recorded
library, and a failure prints it."""
import hashlib
import json
import os

import pytest
import torch

import test_gpu_branch_depth as bd
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = bd.DEV
L = 2
MS = (1, 17, 77, 531, 1100)
NCS = (1, 10, 26, 64)
DIMS = (bd.DEFAULT, (10,), (1,) * 10)
FIXTURE = os.path.join(GOLDEN, 'branches_parent_bits.json')


def _dt(M, per_row):
    """(dt, dt_rows): per row 0.5 / 0 / 0.25 by row index (a zero leaves the velocity undivided), or the scalar 0.5"""
    if not per_row:
        return 0.5, None
    return 0.0, torch.tensor([0.5, 0.0, 0.25])[torch.arange(M) % 3].to(DEV)


def _digest(t):
    """what the fixture keeps of an output tensor"""
    a = t.detach().cpu().contiguous().view(-1)
    return {'sha256': hashlib.sha256(a.numpy().tobytes()).hexdigest(), 'first8': [float(v) for v in a[:8]], 'last8': [float(v) for v in a[-8:]]}


class _Out:
    """an output [L, M, cols] in a guarded buffer"""

    def __init__(self, M, cols):
        self.n = L * M * cols
        self.buf, flat = bd._guarded(self.n)
        self.t = flat.view(L, M, cols)

    def digest(self):
        torch.cuda.synchronize()
        assert bool((self.buf[self.n:] == bd.SENTINEL).all()), 'a write past the output'
        return _digest(self.t)


def _per_layer_heads(sd, NC):
    """the tables of mv2d_heads_fused_x3(_nc) / mv2d_heads_cls_x3_nc from a depth-2 state"""
    from mv2d_amd import ops
    st = lambda fmt: torch.stack([sd[fmt.format(l)] for l in range(L)]).contiguous().to(DEV)
    c = {k: st('cls_branches.{}.' + k) for k in ('0.weight', '0.bias', '1.weight', '1.bias', '3.weight', '3.bias', '4.weight', '4.bias',
                                                 '6.weight', '6.bias')}
    r = {k: st('reg_branches.{}.' + k) for k in ('0.weight', '0.bias', '2.weight', '2.bias', '4.weight', '4.bias')}
    cw = [*ops.pack_x3_stack(c['0.weight']), c['0.bias'], c['1.weight'], c['1.bias'], *ops.pack_x3_stack(c['3.weight']), c['3.bias'], c['4.weight'],
          c['4.bias'], c['6.weight'], c['6.bias']]
    rw = [*ops.pack_x3_stack(r['0.weight']), r['0.bias'], *ops.pack_x3_stack(r['2.weight']), r['2.bias'], r['4.weight'], r['4.bias']]
    return cw, rw


def _per_layer_reg_layer(sd, dims):
    """the table of mv2d_reg_layer_x3 from a depth-2 RegLayer state"""
    from mv2d_amd import ops
    G = len(dims)
    s1 = lambda fmt: torch.stack([sd['reg_branches.' + fmt.format(l)] for l in range(L)]).to(DEV)
    sg = lambda fmt, join: torch.stack([join([sd['reg_branches.' + fmt.format(l, g)] for g in range(G)]) for l in range(L)]).to(DEV)
    return ops.pack_reg_layer(s1('{}.reg_branch.0.weight'), s1('{}.reg_branch.0.bias'), s1('{}.reg_branch.3.weight'), s1('{}.reg_branch.3.bias'),
                              sg('{}.task_heads.{}.0.weight', torch.stack), sg('{}.task_heads.{}.0.bias', torch.stack),
                              sg('{}.task_heads.{}.2.weight', torch.cat), sg('{}.task_heads.{}.2.bias', torch.cat))


def heads_digests(M, NC):
    """{case id: digest} of the five heads entries at (M, NC): the depth entries at n = 1, 2, 3, the first entries at depth 2"""
    from mv2d_amd import ops
    outs, ref, _ = (t.to(DEV) for t in bd._rows(M, L))
    dt, dt_rows = _dt(M, (MS.index(M) + NCS.index(NC)) % 2 == 0)
    pcr, got = bd._pcr(), {}
    for n in (1, 2, 3):
        _, cls_t, reg_t = bd._tables(L, n, NC)
        cp, rp = ops.make_ptr_array(cls_t), ops.make_ptr_array(reg_t)
        cls, reg, cls1 = _Out(M, NC), _Out(M, 10), _Out(M, NC)
        ops.heads_depth_x3(outs, cp, rp, ref, cls.t, reg.t, M, L, n, pcr, dt=dt, dt_rows=dt_rows, num_classes=NC)
        ops.heads_cls_depth_x3(outs, cp, cls1.t, M, L, n, num_classes=NC)
        got.update({f'heads_depth_x3/M{M}/NC{NC}/n{n}/cls': cls.digest(), f'heads_depth_x3/M{M}/NC{NC}/n{n}/reg': reg.digest(),
                    f'heads_cls_depth_x3/M{M}/NC{NC}/n{n}/cls': cls1.digest()})
    cw, rw = _per_layer_heads(bd._tables(L, 2, NC)[0], NC)
    cls, reg, cls1 = _Out(M, NC), _Out(M, 10), _Out(M, NC)
    # (num_classes = 10 goes to mv2d_heads_fused_x3, every other count to mv2d_heads_fused_x3_nc)
    ops.heads_fused_x3(outs, ops.make_ptr_array(cw), ops.make_ptr_array(rw), ref, cls.t, reg.t, M, L, pcr, dt=dt, dt_rows=dt_rows, num_classes=NC)
    ops.heads_cls_x3(outs, ops.make_ptr_array(cw), cls1.t, M, L, num_classes=NC)
    entry = 'heads_fused_x3' if NC == 10 else 'heads_fused_x3_nc'
    got.update({f'{entry}/M{M}/NC{NC}/cls': cls.digest(), f'{entry}/M{M}/NC{NC}/reg': reg.digest(), f'heads_cls_x3_nc/M{M}/NC{NC}/cls': cls1.digest()})
    return got


def reg_layer_digests(M, dims):
    """{case id: digest} of the two RegLayer entries at (M, group layout): the depth entry at n = 1, 2, 3, the first entry at depth 2"""
    from mv2d_amd import ops
    outs, ref, _ = (t.to(DEV) for t in bd._rows(M, L))
    dt, dt_rows = _dt(M, (MS.index(M) + DIMS.index(dims)) % 2 == 1)
    pcr, got, g = bd._pcr(), {}, 'g' + ''.join(map(str, dims))
    for n in (1, 2, 3):
        reg = _Out(M, 10)
        ops.reg_layer_depth_x3(outs, ops.make_ptr_array(bd._tables(L, n, 10, dims)[2]), ref, reg.t, M, L, n, dims, pcr, dt=dt, dt_rows=dt_rows)
        got[f'reg_layer_depth_x3/M{M}/{g}/n{n}/reg'] = reg.digest()
    reg = _Out(M, 10)
    ops.reg_layer_x3(outs, ops.make_ptr_array(_per_layer_reg_layer(bd._tables(L, 2, 10, dims)[0], dims)), ref, reg.t, M, L, dims, pcr, dt=dt,
                     dt_rows=dt_rows)
    got[f'reg_layer_x3/M{M}/{g}/reg'] = reg.digest()
    return got


def digests():
    """every case of this module, as the fixture's "cases" (recording: README_branches_parent_bits.md)"""
    got = {}
    for M in MS:
        for NC in NCS:
            got.update(heads_digests(M, NC))
        for dims in DIMS:
            got.update(reg_layer_digests(M, dims))
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


@pytest.mark.parametrize('NC', NCS)
@pytest.mark.parametrize('M', MS)
def test_heads_entries_write_the_parent_bits(M, NC):
    _check(heads_digests(M, NC))


@pytest.mark.parametrize('dims', DIMS, ids=lambda d: 'g' + ''.join(map(str, d)))
@pytest.mark.parametrize('M', MS)
def test_reg_layer_entries_write_the_parent_bits(M, dims):
    _check(reg_layer_digests(M, dims))


def test_fixture_lists_exactly_these_cases():
    with open(FIXTURE) as fh:
        fixture = json.load(fh)
    heads = {f'{e}/M{M}/NC{NC}/n{n}/{o}' for M in MS for NC in NCS for n in (1, 2, 3)
             for e, o in (('heads_depth_x3', 'cls'), ('heads_depth_x3', 'reg'), ('heads_cls_depth_x3', 'cls'))}
    heads |= {f'{e}/M{M}/NC{NC}/{o}' for M in MS for NC in NCS
              for e, o in (('heads_fused_x3' if NC == 10 else 'heads_fused_x3_nc', 'cls'), ('heads_fused_x3' if NC == 10 else 'heads_fused_x3_nc', 'reg'),
                           ('heads_cls_x3_nc', 'cls'))}
    regl = {f'reg_layer_depth_x3/M{M}/g{"".join(map(str, d))}/n{n}/reg' for M in MS for d in DIMS for n in (1, 2, 3)}
    regl |= {f'reg_layer_x3/M{M}/g{"".join(map(str, d))}/reg' for M in MS for d in DIMS}
    assert set(fixture['cases']) == heads | regl and fixture['hipcc_version']
    assert {k.split('/')[0] for k in fixture['cases']} == {'heads_fused_x3', 'heads_fused_x3_nc', 'heads_cls_x3_nc', 'reg_layer_x3', 'heads_depth_x3',
                                                          'heads_cls_depth_x3', 'reg_layer_depth_x3'}
