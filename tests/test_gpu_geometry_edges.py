"""The frame-geometry kernels of csrc/geometry.hip against oracle/mv2d_oracle.py on the edge problems of tests/geometry_cases.py (-m gpu):
views of more than 128 / 256 RoIs, empty views, R = 1 / 127 / 128 / 129, duplicate, tiny, border and outside boxes, a two-sample batch, and
the sampling keys of box_correlation off their defaults.  Every integer output, K_roi and intr are compared exactly -- `match` position by
position, dropped entries included; minv with the bound of test_gpu_kernels.py::test_box_params_roialign_refpoint.
tests/test_geometry_cases_cpu.py shows what these comparisons can tell apart."""
import functools
import types

import numpy as np
import pytest
import torch

import geometry_cases as gc

pytestmark = pytest.mark.gpu

SENTINEL = -7


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    from mv2d_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def relerr(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


@functools.lru_cache(maxsize=None)
def _on_device(name, dev):
    c = gc.make_case(name)
    return types.SimpleNamespace(rois=c.rois.to(dev), view_start=c.view_start.to(dev), trans=c.trans.to(dev), viewK=c.viewK.to(dev),
                                 viewE=c.viewE.to(dev), pad_mask=c.pad_mask.to(dev))


@functools.lru_cache(maxsize=None)
def _tables_on_device(sampling, dev):
    t = gc.tables(gc.params(sampling + (0.0, 0.0, 1)))
    return t['lin'].to(dev), t['depths'].to(dev)


def _keys(p):
    return dict(sample_size=p.sample_size, num_depth=p.num_depth, depth_start=p.depth_start, iou_thr=p.iou_thr, ratio=p.ratio)


def _box_correlation(dev, name, ps, rois=None, view_start=None, trans=None, R=None, max_per_view=None):
    """match [R, V, topk] of mv2d_box_correlation on a sentinel-filled buffer"""
    from mv2d_amd import ops
    c, d, p = gc.make_case(name), _on_device(name, dev), gc.params(ps)
    lin, depths = _tables_on_device(ps[:3], dev)
    rois = d.rois if rois is None else rois
    match = torch.full((rois.shape[0], c.V, p.topk), SENTINEL, dtype=torch.int32, device=dev)
    ops.box_correlation(rois, d.view_start if view_start is None else view_start, d.trans if trans is None else trans, lin, depths, match, c.V,
                        p.topk, c.pad_h, c.pad_w, c.max_per_view if max_per_view is None else max_per_view, **_keys(p))
    return match


@pytest.mark.parametrize('name', ['mid_empty', 'r1', 'batch'])
def test_box_params_roi_size_scale_and_min_size(dev, name):
    from mv2d_amd import ops
    c, d = gc.make_case(name), _on_device(name, dev)
    R = c.R
    for s, intr_scale, min_size in ((1, 0.1, 4), (7, 1.0, 0), (14, 0.1, 16), (7, 0.1, 4)):
        K_ref, E_ref = gc.box_params_ref(c, s)
        K_roi = torch.empty((R, 16), dtype=torch.float64, device=dev)
        intr = torch.full((R, 32), 123.0, device=dev)
        minv = torch.empty((R, 16), device=dev)
        ops.box_params(d.rois, d.viewK, d.viewE, intr, 32, minv, K_roi=K_roi, roi_size=float(s), intr_scale=intr_scale, min_size=float(min_size))
        assert torch.equal(K_roi.cpu().view(R, 4, 4), K_ref), f'K_roi at roi_size {s}'
        assert torch.equal(intr[:, :16].cpu(), gc.intr_ref(c, K_ref, intr_scale, min_size)), f'intr at {(s, intr_scale, min_size)}'
        assert bool((intr[:, 16:] == 123.0).all()), 'the tail of the ld_intr = 32 rows was written'
        minv_ref = torch.inverse(torch.bmm(K_ref, E_ref.transpose(1, 2))).float()
        assert relerr(minv.view(R, 4, 4), minv_ref) < 1e-6
    if 'clamp' in c.special:
        assert float(intr[c.special['w3'][0], :16].abs().max()) == 0.0


@pytest.mark.parametrize('ps', gc.PARAM_SETS, ids=lambda ps: '-'.join(str(x) for x in ps))
@pytest.mark.parametrize('name', list(gc.LAYOUTS))
def test_box_correlation_position_wise(dev, name, ps):
    """match[r, v, rank] is the oracle's id where the oracle keeps the entry and -1 where it drops it, -1 behind the list, in the RoI's own view
    and in views without RoIs; nothing of the sentinel is left."""
    exp, _ = gc.expected_match(name, ps)
    got = _box_correlation(dev, name, ps).cpu()
    bad = (got != exp).view(exp.shape[0], -1).any(1)
    assert not bool(bad.any()), f'{int(bad.sum())}/{exp.shape[0]} RoIs with a different match row, first: RoI {int(bad.nonzero()[0])}'


@pytest.mark.parametrize('ps', [gc.PARAM_SETS[0], gc.PARAM_SETS[3], gc.PARAM_SETS[4]], ids=lambda ps: '-'.join(str(x) for x in ps))
def test_batch_equals_single_sample_launches(dev, ps):
    c, d = gc.make_case('batch'), _on_device('batch', dev)
    both = _box_correlation(dev, 'batch', ps).cpu()
    assert c.B == 2
    for b, s in enumerate(c.samples):
        n = s.rois.shape[0]
        vs = torch.tensor(np.concatenate([[0], np.cumsum(s.npv)]), dtype=torch.int32, device=dev)
        one = _box_correlation(dev, 'batch', ps, rois=s.rois.to(dev), view_start=vs, trans=d.trans[b * c.V:(b + 1) * c.V].contiguous(),
                               max_per_view=max(s.npv)).cpu()
        one = torch.where(one >= 0, one + s.first, one)
        assert torch.equal(both[s.first:s.first + n], one), f'sample {b}'


ZERO_BYTES = (None, 16, 16 * 1024, 16 * 1024 + 16)
GUARD = 64


@pytest.mark.parametrize('name', ['r1', 'r127', 'r128', 'r129', 'mid_empty'])
def test_frame_geometry_equals_its_parts(dev, name):
    from mv2d_amd import ops
    c, d = gc.make_case(name), _on_device(name, dev)
    R = c.R
    runs = ((gc.PARAM_SETS[4], 14.0, 1.0, 16.0), (gc.PARAM_SETS[1], 7.0, 0.1, 4.0), (gc.PARAM_SETS[3], 1.0, 1.0, 0.0), (gc.PARAM_SETS[2], 7.0, 0.1, 0.0))
    for zero_bytes, (ps, roi_size, intr_scale, min_size) in zip(ZERO_BYTES, runs):
        p = gc.params(ps)
        lin, depths = _tables_on_device(ps[:3], dev)
        K0 = torch.empty((R, 16), dtype=torch.float64, device=dev)
        intr0 = torch.full((R, 32), 123.0, device=dev)
        minv0 = torch.empty((R, 16), device=dev)
        ops.box_params(d.rois, d.viewK, d.viewE, intr0, 32, minv0, K_roi=K0, roi_size=roi_size, intr_scale=intr_scale, min_size=min_size)
        match0 = _box_correlation(dev, name, ps)
        K1 = torch.empty_like(K0)
        intr1 = torch.full((R, 32), 123.0, device=dev)
        minv1 = torch.empty_like(minv0)
        match1 = torch.full_like(match0, SENTINEL)
        buf = torch.full(((zero_bytes or 0) + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
        ops.frame_geometry(d.rois, d.viewK, d.viewE, intr1, 32, minv1, d.view_start, d.trans, lin, depths, match1, c.V, p.topk, c.pad_h, c.pad_w,
                           c.max_per_view, K_roi=K1, roi_size=roi_size, intr_scale=intr_scale, min_size=min_size,
                           zero=None if zero_bytes is None else buf[:zero_bytes], **_keys(p))
        assert torch.equal(K1.view(torch.int64), K0.view(torch.int64)), (zero_bytes, 'K_roi')
        assert torch.equal(intr1.view(torch.int32), intr0.view(torch.int32)), (zero_bytes, 'intr')
        assert torch.equal(minv1.view(torch.int32), minv0.view(torch.int32)), (zero_bytes, 'minv')
        assert torch.equal(match1, match0), (zero_bytes, 'match')
        n = zero_bytes or 0
        assert bool((buf[:n] == 0).all()) and bool((buf[n:] == 0xFF).all()), f'cleared region of {n} bytes'


@pytest.mark.parametrize('zero_bytes', ZERO_BYTES)
def test_frame_geometry_without_rois_only_clears(dev, zero_bytes):
    from mv2d_amd import ops
    c, d = gc.make_case('r127'), _on_device('r127', dev)
    p = gc.params(gc.PARAM_SETS[0])
    lin, depths = _tables_on_device(gc.PARAM_SETS[0][:3], dev)
    K = torch.full((4, 16), 5.0, dtype=torch.float64, device=dev)
    intr = torch.full((4, 32), 123.0, device=dev)
    minv = torch.full((4, 16), 123.0, device=dev)
    match = torch.full((4, c.V, p.topk), SENTINEL, dtype=torch.int32, device=dev)
    buf = torch.full(((zero_bytes or 0) + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    vs = torch.zeros(c.V + 1, dtype=torch.int32, device=dev)
    ops.frame_geometry(d.rois, d.viewK, d.viewE, intr, 32, minv, vs, d.trans, lin, depths, match, c.V, p.topk, c.pad_h, c.pad_w, 0,
                       K_roi=K, zero=None if zero_bytes is None else buf[:zero_bytes], R=0)
    n = zero_bytes or 0
    assert bool((buf[:n] == 0).all()) and bool((buf[n:] == 0xFF).all())
    assert bool((K == 5.0).all()) and bool((intr == 123.0).all()) and bool((minv == 123.0).all()) and bool((match == SENTINEL).all())


# (topk, expand_stride) in (1, 0), (20, 2), (300, 2) and one more set with iou_thr > 0 (the third has one too)
T_RUNS = ((gc.PARAM_SETS[7], 0), (gc.PARAM_SETS[0], 2), (gc.PARAM_SETS[3], 2), (gc.PARAM_SETS[1], 2))


def _mask_compact(dev, name, ps, expand, match, col_len, col_cap=None):
    from mv2d_amd import ops
    c, d, p = gc.make_case(name), _on_device(name, dev), gc.params(ps)
    R, V, h, w = c.R, c.V, c.h, c.w
    P = V * h * w
    o = types.SimpleNamespace(
        roi_mask=torch.zeros(P, dtype=torch.uint8, device=dev), rect=torch.empty((R, 5), dtype=torch.int32, device=dev),
        pos2s=torch.empty(P, dtype=torch.int32, device=dev), s2pos=torch.empty(P, dtype=torch.int32, device=dev),
        S_out=torch.zeros(1, dtype=torch.int32, device=dev), row_count=torch.empty(R, dtype=torch.int32, device=dev),
        row_ptr=torch.empty(R + 1, dtype=torch.int32, device=dev), col=torch.full((col_len,), SENTINEL, dtype=torch.int32, device=dev),
        nnz=torch.zeros(2, dtype=torch.int32, device=dev))
    bits = torch.empty(ops.csr_workspace_bytes(R, V, h, w) // 4, dtype=torch.int32, device=dev)
    ops.mask_compact(d.rois, match, d.pad_mask, o.roi_mask, o.rect, o.pos2s, o.s2pos, o.S_out, bits, o.row_count, o.row_ptr, o.col, o.nnz, R, V, h, w,
                     p.topk, float(gc.STRIDE), float(expand), col_cap=col_cap)
    return o


@pytest.mark.parametrize('ps,expand', T_RUNS, ids=lambda x: '-'.join(str(y) for y in x) if isinstance(x, tuple) else str(x))
@pytest.mark.parametrize('name', ['mid_empty', 'first_empty'])
def test_t_path_masks_and_csr(dev, name, ps, expand):
    from oracle import mv2d_oracle as O
    c = gc.make_case(name)
    R, V, h, w = c.R, c.V, c.h, c.w
    ffr, pad = gc.t_path_ref(name, ps, expand)
    assert torch.equal(c.pad_mask.bool().view(V, h, w), pad)
    keep = (ffr.any(0) & ~pad).view(-1)
    allowed = (ffr & ~pad[None]).view(R, -1)[:, keep]
    rp_ref, col_ref = O.csr_from_allowed(allowed)
    nnz = int(rp_ref[-1])
    match = _box_correlation(dev, name, ps)
    o = _mask_compact(dev, name, ps, expand, match, nnz + GUARD)
    assert torch.equal(o.roi_mask.cpu().bool().view(V, h, w), ffr.any(0))
    S = int(o.S_out)
    assert S == int(keep.sum())
    assert torch.equal(o.s2pos[:S].cpu().long(), keep.nonzero()[:, 0])
    assert torch.equal(o.row_ptr.cpu(), rp_ref)
    assert int(o.nnz[0]) == nnz and int(o.nnz[1]) == 0
    assert torch.equal(o.col[:nnz].cpu(), col_ref)
    assert bool((o.col[nnz:] == SENTINEL).all())
    if name == 'mid_empty':
        assert int((rp_ref[1:] == rp_ref[:-1]).sum()) > 0                       # (an empty row is among them)
    if (name, expand, ps) == ('mid_empty', 2, gc.PARAM_SETS[0]):
        # csr_fill_kernel: nnz_out[1] = 1 when a row ends beyond col_cap, and nothing is written at or beyond col_cap
        o = _mask_compact(dev, name, ps, expand, match, nnz + GUARD, col_cap=nnz - 1)
        assert int(o.nnz[1]) == 1 and int(o.nnz[0]) == nnz
        assert torch.equal(o.col[:nnz - 1].cpu(), col_ref[:nnz - 1])
        assert bool((o.col[nnz - 1:] == SENTINEL).all())


@pytest.mark.parametrize('name', ['mid_empty', 'r127'])
def test_s_path_csr_skips_the_gaps(dev, name):
    from mv2d_amd import ops
    ps = gc.PARAM_SETS[1]                                                       # iou_thr = 0.3, ratio = 0.5, topk = 5
    c, p = gc.make_case(name), gc.params(ps)
    R, V = c.R, c.V
    rows = [[r] + [i for i, k in row if k] for r, row in enumerate(gc.epipolar(name, ps))]
    match = _box_correlation(dev, name, ps)
    m = match.cpu().view(R, -1)
    assert any(bool((m[r, :int((m[r] >= 0).nonzero().max()) + 1] < 0).any()) for r in range(R) if bool((m[r] >= 0).any())), 'no gap in any row'
    exp_cols = torch.tensor([i * 49 + cell for row in rows for i in row for cell in range(49)], dtype=torch.int32)
    exp_ptr = torch.tensor([0] + [len(row) * 49 for row in rows], dtype=torch.int64).cumsum(0).to(torch.int32)
    row_ptr = torch.empty(R + 1, dtype=torch.int32, device=dev)
    col = torch.full((R * (1 + V * p.topk) * 49,), SENTINEL, dtype=torch.int32, device=dev)
    nnz = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.csr_from_corr(match, row_ptr, col, nnz, R, V, p.topk)
    assert int(nnz) == exp_cols.numel()
    assert torch.equal(row_ptr.cpu(), exp_ptr)
    assert torch.equal(col[:int(nnz)].cpu(), exp_cols)
    assert bool((col[int(nnz):] == SENTINEL).all())
