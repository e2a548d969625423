"""box_correlation's sampling keys and intrins_feat_scale on the GPU (-m gpu).  Kernel level: mv2d_box_correlation_ex and the fused
mv2d_frame_geometry_ex against the reference goldens tests/golden/box_corr_keys_kernel.npz (every parameter set, layouts r127 and mid_empty, exact)
and, for the LID sets, against oracle/mv2d_oracle.py on r1, first_empty, r129 and the two-sample batch; depth_start compared in double; the shipped
keys through the new entries give the bytes of the old entries.  End to end: HeadEngine and the plugin heads on the goldens
box_corr_keys_corr3_*.npz under the bounds of tests/test_gpu_decoder_shape.py.  tests/test_box_corr_keys_cpu.py shows what the goldens hold."""
import functools
import types

import numpy as np
import pytest
import torch

import geometry_cases as gc
from conftest import load_golden, unpack_bits
from mv2d_amd import calib, configs, synthetic
from oracle import mv2d_oracle as O
from test_box_corr_keys_cpu import E2E_KEYS, golden_match, identity_case, key_sets

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7
GUARD = 64
ZERO_BYTES = 16 * 1024 + 16
# tests/test_gpu_decoder_shape.py
TOL_CENTER, TOL_CLS, TOL_BOX = 1.3e-4, 3e-6, 5e-3
KEY_SETS = key_sets()
LID_SETS = [ks for ks in KEY_SETS if ks[4]]
SHIPPED = (4, 8, 0.5, 70.0, True, 20)
_ids = lambda ks: '-'.join(str(x) for x in ks) if isinstance(ks, tuple) else str(ks)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    from mv2d_amd import _lib
    _lib.load()
    return torch.device(DEV)


def relerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


@functools.lru_cache(maxsize=None)
def _on_device(name):
    c = gc.make_case(name)
    return types.SimpleNamespace(rois=c.rois.to(DEV), view_start=c.view_start.to(DEV), trans=c.trans.to(DEV), viewK=c.viewK.to(DEV), viewE=c.viewE.to(DEV))


@functools.lru_cache(maxsize=None)
def _tables(ks):
    t = calib.constant_tables(ks[0], ks[1], ks[2], ks[3], lid=ks[4])
    return t['lin'].to(DEV), t['depths'].to(DEV)


def _corr(name, ks):
    """match of the stand-alone launch on a sentinel-filled buffer"""
    from mv2d_amd import ops
    c, d = gc.make_case(name), _on_device(name)
    lin, depths = _tables(ks)
    match = torch.full((c.R, c.V, ks[5]), SENTINEL, dtype=torch.int32, device=DEV)
    ops.box_correlation(d.rois, d.view_start, d.trans, lin, depths, match, c.V, ks[5], c.pad_h, c.pad_w, c.max_per_view, sample_size=ks[0],
                        num_depth=ks[1], depth_start=ks[2])
    return match


def _frame(name, ks, intr_scale=0.1):
    """(match, K_roi, intr, minv, buf) of the fused frame launch; buf: ZERO_BYTES to clear + GUARD bytes that must stay"""
    from mv2d_amd import ops
    c, d = gc.make_case(name), _on_device(name)
    lin, depths = _tables(ks)
    o = types.SimpleNamespace(match=torch.full((c.R, c.V, ks[5]), SENTINEL, dtype=torch.int32, device=DEV),
                              K=torch.empty((c.R, 16), dtype=torch.float64, device=DEV), intr=torch.full((c.R, 32), 123.0, device=DEV),
                              minv=torch.empty((c.R, 16), device=DEV), buf=torch.full((ZERO_BYTES + GUARD,), 0xFF, dtype=torch.uint8, device=DEV))
    ops.frame_geometry(d.rois, d.viewK, d.viewE, o.intr, 32, o.minv, d.view_start, d.trans, lin, depths, o.match, c.V, ks[5], c.pad_h, c.pad_w,
                       c.max_per_view, K_roi=o.K, intr_scale=intr_scale, zero=o.buf[:ZERO_BYTES], sample_size=ks[0], num_depth=ks[1], depth_start=ks[2])
    return o


@functools.lru_cache(maxsize=None)
def _oracle_match(name, ks):
    case = gc.make_case(name)
    ep = []
    for s in case.samples:
        rows = O.epipolar_in_box(s.rois, s.npv, s.metas[0]['pad_shape'], O.view_transforms(s.metas), ks[5], 0.0, 0.0, ks[0], ks[1], ks[2], ks[3])
        ep += [[(i + s.first, k) for i, k in row] for row in rows]
    return gc.match_from_lists(case, ep, ks[5])[0].numpy()


# ------------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize('ks', KEY_SETS, ids=_ids)
@pytest.mark.parametrize('name', ['r127', 'mid_empty'])
def test_both_launch_forms_equal_the_reference_golden(dev, name, ks):
    """... and each other; the cameras and the cleared bytes of the fused launch are those of the launch at the shipped keys."""
    want = golden_match(name, ks)
    got = _corr(name, ks).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    f = _frame(name, ks)
    np.testing.assert_array_equal(f.match.cpu().numpy(), want)
    s = _frame(name, SHIPPED)
    assert torch.equal(f.K.view(torch.int64), s.K.view(torch.int64)) and torch.equal(f.intr.view(torch.int32), s.intr.view(torch.int32))
    assert torch.equal(f.minv.view(torch.int32), s.minv.view(torch.int32))
    assert bool((f.buf[:ZERO_BYTES] == 0).all()) and bool((f.buf[ZERO_BYTES:] == 0xFF).all())
    assert bool((f.intr[:, 16:] == 123.0).all())


@pytest.mark.parametrize('ks', LID_SETS, ids=_ids)
@pytest.mark.parametrize('name', ['r1', 'first_empty', 'r129', 'batch'])
def test_both_launch_forms_equal_the_oracle(dev, name, ks):
    want = _oracle_match(name, ks)
    np.testing.assert_array_equal(_corr(name, ks).cpu().numpy(), want)
    np.testing.assert_array_equal(_frame(name, ks).match.cpu().numpy(), want)


@pytest.mark.parametrize('name', ['r127', 'mid_empty', 'batch'])
def test_shipped_keys_through_the_ex_entries_give_the_bytes_of_the_old_entries(dev, name):
    from mv2d_amd import _lib, ops
    from mv2d_amd.ops import _p, _stream
    lib = _lib.load()
    c, d = gc.make_case(name), _on_device(name)
    for ks in (SHIPPED, (4, 8, 0.5, 70.0, True, 1), (2, 32, 1.0, 70.0, True, 5)):
        lin, depths = _tables(ks)
        old = torch.full((c.R, c.V, ks[5]), SENTINEL, dtype=torch.int32, device=DEV)
        assert lib.mv2d_box_correlation(_p(d.rois), _p(d.view_start), _p(d.trans), _p(lin), _p(depths), _p(old), c.R, c.V, ks[0], ks[1], ks[5], c.pad_h,
                                        c.pad_w, ks[2], 0.0, 0.0, c.max_per_view, _stream()) == 0
        assert torch.equal(_corr(name, ks), old)
        assert torch.equal(old.cpu(), torch.from_numpy(_oracle_match(name, ks)))
        f = _frame(name, ks)
        o = types.SimpleNamespace(match=torch.full_like(old, SENTINEL), K=torch.empty_like(f.K), intr=torch.full_like(f.intr, 123.0),
                                  minv=torch.empty_like(f.minv), buf=torch.full_like(f.buf, 0xFF))
        assert lib.mv2d_frame_geometry(_p(d.rois), _p(d.viewK), _p(d.viewE), _p(o.K), _p(o.intr), 32, _p(o.minv), 7.0, 0.1, 4.0, _p(d.view_start),
                                       _p(d.trans), _p(lin), _p(depths), _p(o.match), c.R, c.V, ks[0], ks[1], ks[5], c.pad_h, c.pad_w, ks[2], 0.0, 0.0,
                                       c.max_per_view, _p(o.buf), ZERO_BYTES, _stream()) == 0
        assert torch.equal(o.match, old) and torch.equal(f.match, old)
        assert torch.equal(f.K.view(torch.int64), o.K.view(torch.int64)) and torch.equal(f.intr.view(torch.int32), o.intr.view(torch.int32))
        assert torch.equal(f.minv.view(torch.int32), o.minv.view(torch.int32)) and torch.equal(f.buf, o.buf)


def test_both_instances_agree_where_depth_start_cannot_matter(dev):
    """64, 128 and 128 samples at depth_start 0.5 run the first instance.  The same keys at 0.5 + 1e-9, which is no fp32 number, run the second; no
    camera depth of the case lies between the two values, so the lists must be equal."""
    from mv2d_amd import ops
    c, d = gc.make_case('r129'), _on_device('r129')
    ds = 0.5 + 1e-9
    assert float(np.float32(ds)) != ds
    for ss, D in ((1, 64), (8, 2), (4, 8)):
        ks = (ss, D, 0.5, 70.0, True, 20)
        lin, depths = _tables(ks)
        b = torch.full((c.R, c.V, 20), SENTINEL, dtype=torch.int32, device=DEV)
        ops.box_correlation(d.rois, d.view_start, d.trans, lin, depths, b, c.V, 20, c.pad_h, c.pad_w, c.max_per_view, sample_size=ss, num_depth=D,
                            depth_start=ds)
        assert torch.equal(_corr('r129', ks), b), (ss, D)
        np.testing.assert_array_equal(b.cpu().numpy(), _oracle_match('r129', ks))


@pytest.mark.parametrize('depth_start,matched', [(0.7, False), (0.9, False), (0.5, True), (0.3, True)])
def test_depth_start_is_compared_in_double(dev, depth_start, matched):
    """16 samples, so the first instance would serve: 0.7, 0.9 and 0.3 are no fp32 numbers and must go to the instance that compares in double.
    fp32(0.7) < 0.7: no sample is valid, all -1; an fp32 compare would match the two boxes."""
    from mv2d_amd import ops
    rois, npv, shape, trans = identity_case()
    t = calib.constant_tables(4, 1, depth_start, 70)
    vs = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    args = (vs, trans.reshape(2, 2, 16).to(DEV), t['lin'].to(DEV), t['depths'].to(DEV))
    want = torch.tensor([[[-1], [1]], [[0], [-1]]] if matched else [[[-1], [-1]], [[-1], [-1]]], dtype=torch.int32)
    match = torch.full((2, 2, 1), SENTINEL, dtype=torch.int32, device=DEV)
    ops.box_correlation(rois.to(DEV), *args, match, 2, 1, shape[0], shape[1], 1, sample_size=4, num_depth=1, depth_start=depth_start)
    assert torch.equal(match.cpu(), want)
    K = torch.eye(4, dtype=torch.float64).reshape(1, 16).repeat(2, 1).to(DEV)
    match2 = torch.full_like(match, SENTINEL)
    ops.frame_geometry(rois.to(DEV), K, K, torch.empty((2, 16), device=DEV), 16, torch.empty((2, 16), device=DEV), *args, match2, 2, 1, shape[0],
                       shape[1], 1, sample_size=4, num_depth=1, depth_start=depth_start)
    assert torch.equal(match2.cpu(), want)


@pytest.mark.parametrize('ss,D', [(0, 8), (9, 1), (4, 0), (1, 65), (-1, 8)])
def test_c_entries_refuse_out_of_range_keys(dev, ss, D):
    from mv2d_amd import _lib, ops
    c, d = gc.make_case('r1'), _on_device('r1')
    lin, depths = _tables(SHIPPED)
    match = torch.full((c.R, c.V, 1), SENTINEL, dtype=torch.int32, device=DEV)
    key = 'sample_size' if not 1 <= ss <= 8 else 'num_depth'
    with pytest.raises(_lib.Mv2dHipError, match=key):
        ops.box_correlation(d.rois, d.view_start, d.trans, lin, depths, match, c.V, 1, c.pad_h, c.pad_w, c.max_per_view, sample_size=ss, num_depth=D)
    with pytest.raises(_lib.Mv2dHipError, match=key):
        ops.frame_geometry(d.rois, d.viewK, d.viewE, torch.empty((c.R, 16), device=DEV), 16, torch.empty((c.R, 16), device=DEV), d.view_start, d.trans,
                           lin, depths, match, c.V, 1, c.pad_h, c.pad_w, c.max_per_view, sample_size=ss, num_depth=D)
    assert bool((match == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------ engine and heads
_RN = load_golden('box_corr_keys_refnoise')
CASES = {'corr3_s_keys': ('corr3_s', E2E_KEYS, 0.05), 'corr3_t_keys': ('corr3_t', E2E_KEYS, 0.05), 'corr3_s_scale': ('corr3_s', None, 0.25)}


@functools.lru_cache(maxsize=None)
def _state():
    """make_head_state(seed=0): drawn once, shared, never written"""
    return synthetic.make_head_state(seed=0)


def _engine_keys(keys, scale):
    kw = dict(intrins_feat_scale=scale)
    if keys is not None:
        kw.update(sample_size=keys['sample_size'], num_depth=keys['num_depth'], corr_depth_start=keys['depth_start'], corr_depth_end=keys['depth_end'],
                  corr_LID=keys['LID'])
    return kw


def _engine(prob, **kw):
    from mv2d_amd.engine import HeadEngine
    return HeadEngine(_state(), prob['kind'], torch.device(DEV), num_views=prob['views_per_frame'], **kw)


def _inputs(prob):
    return torch.from_numpy(prob['feat']).to(DEV), [torch.from_numpy(np.asarray(p)) for p in prob['proposals']], prob['img_metas']


def _all_outputs(eng, out):
    R = out['R']
    return [out['cls'][:, :R].clone(), out['reg'][:, :R].clone(), out['ws']['match'][:R].clone(), out['ws']['intr'][:R, :16].clone()] + \
        [t.clone() for t in eng.results(out)]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _ranks_vs_golden(flat, g, noise):
    ref = g['topk_index']
    assert len(ref) == len(flat)
    n_idx = int((flat != ref).sum())
    assert n_idx <= noise, (n_idx, noise)
    pos = {int(v): j for j, v in enumerate(ref)}
    for i, v in enumerate(flat):
        if int(v) != int(ref[i]):
            j = pos.get(int(v))
            assert j is not None and abs(float(g['topk_scores'][i]) - float(g['topk_scores'][j])) <= 1e-7, (i, int(v))
    return n_idx


@pytest.mark.parametrize('case', list(CASES))
def test_engine_and_plugin_match_the_reference_golden(case):
    """HeadEngine.run on the index-exact route: intr bit for bit, the key lists exactly, centre / cls / ranked decode under the bounds of
    test_engine_and_plugin_match_reference_golden_decoder_shape and the reference's own rank noise; eager == graph replay and a two-sample batch
    == the single runs, bit for bit; then the plugin head built from the case's config."""
    import mv2d_amd
    problem, keys, scale = CASES[case]
    g = load_golden('box_corr_keys_' + case)
    noise, gap = int(_RN[case + '_pairwise_ranked_diff'].max()), float(_RN[case + '_max_tie_gap'])
    prob = synthetic.make_problem(problem, seed=int(g['seed']))
    eng = _engine(prob, exact=True, **_engine_keys(keys, scale))
    ins = _inputs(prob)
    out = eng.run(*ins, keep_stages=True)
    torch.cuda.synchronize()
    R, st, ws, s = out['R'], out['stages'], out['ws'], 7
    np.testing.assert_array_equal(ws['intr'][:R, :16].cpu().numpy(), g['intr'])
    e_c, e_x = relerr(st['center'][:R], g['center_pred']), relerr(st['xyz'][:R], g['xyz'])
    print(f'[box_corr_keys] {case}: center rel err {e_c:.2e}, xyz rel err {e_x:.2e} (bound {TOL_CENTER:.1e})')
    assert e_c < TOL_CENTER and e_x < TOL_CENTER
    rp, ci = st['row_ptr'].cpu().numpy(), st['col_idx'].cpu().numpy()
    if prob['kind'] == 'T':
        ffr = unpack_bits(g['feat_for_rois'], g['feat_for_rois_shape'])
        roi_mask = ffr.any(0).reshape(-1)
        np.testing.assert_array_equal(st['roi_mask'].cpu().numpy().astype(bool), roi_mask)
        assert int(st['S_dev'].item()) == int(roi_mask.sum())
        allowed = ffr.reshape(R, -1)[:, roi_mask] & ~g['key_padding'][None]
        for r in range(R):
            np.testing.assert_array_equal(np.sort(ci[rp[r]:rp[r + 1]]), np.nonzero(allowed[r])[0])
    else:
        for r in range(R):
            ids = g['corr'][r][g['corr_mask'][r]]
            want = np.sort(np.concatenate([np.arange(s * s) + s * s * int(i) for i in ids]))
            np.testing.assert_array_equal(np.sort(ci[rp[r]:rp[r + 1]]), want)
    e_cls = relerr(out['cls'][:, :R].reshape(g['cls'].shape), g['cls'])
    n = int(out['count'].item())
    labels = out['labels'][:n].cpu().numpy()
    print(f'[box_corr_keys] {case}: cls rel err {e_cls:.2e} (bound {TOL_CLS:.0e}), reference against itself: {noise} ranked indices, gap {gap:.1e}')
    assert e_cls < TOL_CLS, e_cls
    assert n == len(g['labels'])
    n_idx = _ranks_vs_golden(out['bbox_index'][:n].cpu().numpy() * 10 + labels, g, noise)
    print(f'[box_corr_keys] {case}: {n_idx}/{n} ranked (query, class) indices differ')
    # ---- eager == graph replay, a two-sample batch == the single runs
    eager = _all_outputs(eng, eng.run(*ins))
    eng.run(*ins, use_graph=True)                              # capture, then a replay
    _same(_all_outputs(eng, eng.run(*ins, use_graph=True)), eager)
    ob = eng.run_batch([ins[0], ins[0]], [ins[1], ins[1]], [ins[2], ins[2]])
    for res in eng.results_batch(ob):
        _same([t.clone() for t in res], eager[4:])
    # ---- the plugin head: heads.py hands the module's own keys to the engine
    cfg = (configs.roi_head_cfg_s if prob['kind'] == 'S' else configs.roi_head_cfg_t)(box_correlation=keys, intrins_feat_scale=scale)
    if prob['kind'] == 'T':
        cfg['num_views'] = prob['views_per_frame']
    head = mv2d_amd.build_head(cfg, test_cfg=configs.TEST_CFG_RCNN)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in _state().items()}, strict=True)
    head = head.to(DEV).eval()
    metas = [dict(m, box_type_3d=None) for m in prob['img_metas']]
    single = head.simple_test([ins[0]], ins[1], metas)[0]
    peng = head.engine(ins[0].device, metas)
    bc = dict(dict(sample_size=4, num_depth=8, depth_start=0.5, depth_end=70.0, LID=True), **(keys or {}))
    assert (peng.sample_size, peng.num_depth, peng.corr_depth_start, peng.corr_depth_end, peng.corr_LID, peng.intrins_feat_scale) == \
        (bc['sample_size'], bc['num_depth'], bc['depth_start'], bc['depth_end'], bc['LID'], scale)
    boxes, scores, plabels = (t.cpu().numpy() for t in single)
    assert len(plabels) == len(g['labels'])
    assert int((plabels != g['labels']).sum()) <= noise
    assert float(np.abs(scores - g['scores']).max()) <= 0.25 * TOL_CLS * float(np.abs(g['cls']).max())
    po = peng.run(ins[0], ins[1], metas)
    np.testing.assert_array_equal(po['ws']['intr'][:R, :16].cpu().numpy(), g['intr'])
    pidx = po['bbox_index'][:n].cpu().numpy() * 10 + plabels
    _ranks_vs_golden(pidx, g, noise)
    same = pidx == g['topk_index']
    e_box = float(np.abs(boxes - g['boxes'])[same].max() / np.abs(g['boxes']).max())
    print(f'[box_corr_keys] {case}: simple_test boxes rel err {e_box:.2e} (bound {TOL_BOX:.0e})')
    assert e_box < TOL_BOX


def test_module_level_box_correlation_takes_the_keys():
    """BoxCorrelation.gen_box_roi_correlation (the module's own launch, uniform bins through constant_tables(lid=False)) gives the golden's id lists"""
    from mv2d_amd.plugin.modules import BoxCorrelation
    g = load_golden('box_corr_keys_corr3_s_keys')
    prob = synthetic.make_problem('corr3_s', seed=int(g['seed']))
    rois = O.bbox2roi([torch.from_numpy(p) for p in prob['proposals']]).to(DEV)
    m = BoxCorrelation(correlation_mode='topk_matched:1:0.0:0.0', **E2E_KEYS)
    ids, valid = m.gen_box_roi_correlation(rois, [len(p) for p in prob['proposals']], prob['img_metas'])
    ids, valid = ids.cpu().numpy(), valid.cpu().numpy()
    assert valid.shape == g['corr_mask'].shape
    for r in range(rois.shape[0]):
        np.testing.assert_array_equal(ids[r][valid[r]], g['corr'][r][g['corr_mask'][r]])


@pytest.mark.parametrize('exact', [True, False])
@pytest.mark.parametrize('name', ['micro_s', 'micro_t'])
def test_default_keys_run_what_the_engine_ran_before(name, exact):
    """An engine given the shipped keys one by one == an engine given none, bit for bit (tables, match, intr, cls, reg, decode), and its match / intr
    are the bytes of the old C entry on the same RoIs: the shipped keys launch the shipped kernels, whose instruction streams
    tools/cmp_kernel_isa.py holds to the parent's."""
    from mv2d_amd import _lib
    from mv2d_amd.ops import _p, _stream
    prob = synthetic.make_problem(name, seed=0)
    ins = _inputs(prob)
    plain = _engine(prob, exact=exact)
    keyed = _engine(prob, exact=exact, sample_size=4, num_depth=8, corr_depth_start=0.5, corr_depth_end=70, corr_LID=True, intrins_feat_scale=0.1)
    index = torch.arange(0, 8, 1).float()
    depths = (0.5 + ((70.0 - 0.5) / (8 * 9)) * index * (index + 1)).to(DEV)
    for eng in (plain, keyed):
        assert torch.equal(eng.const['depths'], depths) and torch.equal(eng.const['lin'], torch.linspace(0, 1, 4).to(DEV))
    op = plain.run(*ins)
    a = _all_outputs(plain, op)
    _same(_all_outputs(keyed, keyed.run(*ins)), a)
    assert len(a[-1]) > 0
    # the old entry on the engine's own RoIs and tables
    R, ws = op['R'], op['ws']
    V = prob['views_per_frame']
    rois = O.bbox2roi([torch.as_tensor(p) for p in prob['proposals']]).float().contiguous().to(DEV)
    assert rois.shape[0] == R
    geo = calib.geometry_tables(prob['img_metas'])
    npv = [len(p) for p in prob['proposals']]
    vs = torch.tensor(np.concatenate([[0], np.cumsum(npv)]), dtype=torch.int32, device=DEV)
    pad_h, pad_w = prob['img_metas'][0]['pad_shape'][:2]
    match = torch.full((R, V, plain.topk), SENTINEL, dtype=torch.int32, device=DEV)
    intr, minv = torch.empty((R, 16), device=DEV), torch.empty((R, 16), device=DEV)
    lib = _lib.load()
    assert lib.mv2d_frame_geometry(_p(rois), _p(geo['viewK'].to(DEV)), _p(geo['viewE'].to(DEV)), None, _p(intr), 16, _p(minv), 7.0, 0.1, 4.0, _p(vs),
                                   _p(geo['trans'].to(DEV)), _p(plain.const['lin']), _p(plain.const['depths']), _p(match), R, V, 4, 8, plain.topk,
                                   int(pad_h), int(pad_w), 0.5, float(plain.iou_thr), float(plain.ratio), max(npv), None, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(ws['match'][:R].reshape(R, V, plain.topk), match) and torch.equal(ws['intr'][:R, :16], intr)


def test_engine_refuses_the_keys_by_name():
    prob = synthetic.make_problem('micro_s', seed=0)
    for kw, key in ((dict(sample_size=9), r'box_correlation\.sample_size'), (dict(num_depth=8.0), r'box_correlation\.num_depth'),
                    (dict(corr_depth_start=0), r'box_correlation\.depth_start'), (dict(corr_depth_end=0.25), r'box_correlation\.depth_end'),
                    (dict(corr_LID=1), r'box_correlation\.LID'), (dict(intrins_feat_scale=True), 'intrins_feat_scale')):
        with pytest.raises(ValueError, match='HeadEngine: ' + key):
            _engine(prob, **kw)
