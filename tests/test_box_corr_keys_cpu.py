"""box_correlation's sampling keys (sample_size, num_depth, depth_start, depth_end, LID) and intrins_feat_scale without a GPU: the two validators,
the depth tables, the config builders, the plugin modules, the C entries' declarations, and the reference goldens
tests/golden/box_corr_keys_*.npz (tools/gen_golden_box_corr_keys.py) against oracle/mv2d_oracle.py and against the conditions under which they
were recorded.  tests/test_gpu_box_corr_keys.py holds the kernels and the engine to the same goldens."""
import os
import re

import numpy as np
import pytest
import torch

import geometry_cases as gc
from conftest import ROOT, load_golden, unpack_bits
from mv2d_amd import calib, configs, synthetic
from oracle import mv2d_oracle as O

DEFAULT_KEYS = (4, 8, 0.5, 70, True)
E2E_KEYS = dict(sample_size=6, num_depth=16, depth_start=0.3, depth_end=60, LID=False)


def key_sets():
    """rows of the golden's own table: (sample_size, num_depth, depth_start, depth_end, LID, topk)"""
    return [(int(a), int(b), float(c), float(d), bool(e), int(f)) for a, b, c, d, e, f in load_golden('box_corr_keys_kernel')['key_sets']]


def set_name(ks):
    return 'ss%d_d%d_%s_%d_%s_k%d' % (ks[0], ks[1], float(ks[2]), ks[3], 'lid' if ks[4] else 'uni', ks[5])


def golden_match(layout, ks):
    return load_golden('box_corr_keys_kernel')['%s_%s' % (layout, set_name(ks))]


def oracle_match(layout, ks):
    """match [R, V, topk] of oracle.mv2d_oracle.epipolar_in_box (LID depths only) in the form of geometry_cases.match_from_lists"""
    case = gc.make_case(layout)
    s = case.samples[0]
    ep = O.epipolar_in_box(s.rois, s.npv, s.metas[0]['pad_shape'], O.view_transforms(s.metas), ks[5], 0.0, 0.0, ks[0], ks[1], ks[2], ks[3])
    return gc.match_from_lists(case, ep, ks[5])[0].numpy()


# ------------------------------------------------------------------------------------------------------------------------ validators
def test_check_box_correlation_accepts_the_bounds():
    from mv2d_amd import ops
    assert ops.check_box_correlation() == (4, 8, 0.5, 70.0, True)
    assert ops.check_box_correlation(1, 1, 1e-3, 2e-3, False, 'x') == (1, 1, 1e-3, 2e-3, False)
    assert ops.check_box_correlation(8, 64, 1, 1000, True, 'x') == (8, 64, 1.0, 1000.0, True)
    out = ops.check_box_correlation(np.int64(6), np.int32(16), np.float32(0.25), np.float64(60), False, 'x')
    assert out == (6, 16, 0.25, 60.0, False) and [type(v) for v in out] == [int, int, float, float, bool]


@pytest.mark.parametrize('key,bad', [(k, v) for k, vals in (
    ('sample_size', (0, 9, -1, True, 4.0, '4', None)),
    ('num_depth', (0, 65, True, 8.0, '8', None)),
    ('depth_start', (0, -0.5, float('nan'), float('inf'), True, '0.5', None)),
    ('depth_end', (0.5, 0.25, float('inf'), float('nan'), True, '70', None)),
    ('LID', (1, 0, 'True', None))) for v in vals], ids=lambda x: repr(x))
def test_check_box_correlation_refuses_by_the_name_of_the_key(key, bad):
    from mv2d_amd import ops
    with pytest.raises(ValueError, match=r'somebody: box_correlation\.%s ' % key):
        ops.check_box_correlation(who='somebody', **{key: bad})


def test_check_box_correlation_refuses_a_depth_range_that_is_none():
    from mv2d_amd import ops
    for ds, de in ((70, 70), (80.0, 70), (0.5, 0.5)):
        with pytest.raises(ValueError, match=r'somebody: box_correlation\.depth_end must be a finite number > depth_start'):
            ops.check_box_correlation(depth_start=ds, depth_end=de, who='somebody')


def test_check_intrins_feat_scale():
    from mv2d_amd import ops
    assert ops.check_intrins_feat_scale(0.1) == 0.1 and ops.check_intrins_feat_scale(1) == 1.0 and ops.check_intrins_feat_scale(-0.05) == -0.05
    assert type(ops.check_intrins_feat_scale(np.float32(0.25))) is float
    for bad in (True, False, '0.1', None, float('nan'), float('inf'), [0.1]):
        with pytest.raises(ValueError, match='somebody: intrins_feat_scale'):
            ops.check_intrins_feat_scale(bad, 'somebody')


# ------------------------------------------------------------------------------------------------------------------------ tables
def test_constant_tables_uniform_bins_are_torch_linspace():
    for ss, D, ds, de in ((4, 8, 0.5, 70), (6, 16, 0.3, 60), (8, 64, 0.5, 70.0), (1, 1, 0.7, 50)):
        t = calib.constant_tables(ss, D, ds, de, lid=False)
        want = torch.linspace(ds, de, D)
        assert t['depths'].dtype == torch.float32 and torch.equal(t['depths'].view(torch.int32), want.view(torch.int32))
        assert torch.equal(t['lin'], torch.linspace(0, 1, ss))


def test_constant_tables_defaults_are_the_shipped_tables():
    index = torch.arange(0, 8, 1).float()
    depths = 0.5 + ((70.0 - 0.5) / (8 * 9)) * index * (index + 1)
    dim_t = 10000 ** (2 * (torch.arange(128, dtype=torch.float32) // 2) / 128)
    for t in (calib.constant_tables(), calib.constant_tables(lid=True), calib.constant_tables(4, 8, 0.5, 70, lid=True)):
        assert sorted(t) == ['depths', 'dim_t', 'lin']
        assert torch.equal(t['depths'].view(torch.int32), depths.view(torch.int32))
        assert torch.equal(t['lin'].view(torch.int32), torch.linspace(0, 1, 4).view(torch.int32))
        assert torch.equal(t['dim_t'].view(torch.int32), dim_t.view(torch.int32))
    assert not torch.equal(calib.constant_tables(lid=False)['depths'], depths)


# ------------------------------------------------------------------------------------------------------------------------ configs and modules
@pytest.mark.parametrize('kind', ['s', 't'])
def test_configs_lay_the_keys_over_the_shipped_subtree(kind):
    make = configs.roi_head_cfg_s if kind == 's' else configs.roi_head_cfg_t
    shipped = dict(correlation_mode='topk_matched:1:0.0:0.0') if kind == 's' else dict(expand_stride=2, correlation_mode='topk_matched:20:0.0:0.0')
    base = make()
    assert base['box_correlation'] == shipped and 'intrins_feat_scale' not in base
    # the shipped values: no key is added, the dict is the shipped one
    assert make(box_correlation=dict(sample_size=4, num_depth=8, depth_start=0.5, depth_end=70, LID=True), intrins_feat_scale=0.1) == base
    assert make(box_correlation={}) == base and make(box_correlation=None) == base
    d = make(box_correlation=E2E_KEYS, intrins_feat_scale=0.05)
    assert d['box_correlation'] == dict(shipped, **E2E_KEYS) and d['intrins_feat_scale'] == 0.05
    assert {k: v for k, v in d.items() if k not in ('box_correlation', 'intrins_feat_scale')} == {k: v for k, v in base.items() if k != 'box_correlation'}
    d = make(box_correlation=dict(num_depth=16, sample_size=4))
    assert d['box_correlation'] == dict(shipped, num_depth=16) and 'intrins_feat_scale' not in d
    assert make(intrins_feat_scale=0.25)['intrins_feat_scale'] == 0.25 and make(intrins_feat_scale=0.25)['box_correlation'] == shipped
    assert make() == base                                              # (nothing of the calls above stuck to the shipped subtree)
    with pytest.raises(ValueError, match="box_correlation has no key 'depth_num'"):
        make(box_correlation=dict(depth_num=16))
    with pytest.raises(ValueError, match=r'configs: box_correlation\.num_depth'):
        make(box_correlation=dict(num_depth=65))
    with pytest.raises(ValueError, match=r'configs: box_correlation\.depth_end'):
        make(box_correlation=dict(depth_start=2.0, depth_end=1.0))
    with pytest.raises(ValueError, match='configs: intrins_feat_scale'):
        make(intrins_feat_scale=True)


def test_box_correlation_module_takes_the_keys():
    from mv2d_amd.plugin.modules import BoxCorrelation
    m = BoxCorrelation(correlation_mode='topk_matched:20:0.0:0.0', LID=False, force_cpu=True, **{k: v for k, v in E2E_KEYS.items() if k != 'LID'})
    assert (m.sample_size, m.num_depth, m.depth_start, m.depth_end, m.LID, m.topk) == (6, 16, 0.3, 60.0, False, 20)
    m = BoxCorrelation(correlation_mode='topk_matched:1:0.0:0.0')
    assert (m.sample_size, m.num_depth, m.depth_start, m.depth_end, m.LID) == (4, 8, 0.5, 70.0, True)
    for key, bad in (('sample_size', 9), ('num_depth', 8.0), ('depth_start', 0), ('depth_end', 0.25), ('LID', 1)):
        with pytest.raises(ValueError, match=r'BoxCorrelation: box_correlation\.%s ' % key):
            BoxCorrelation(correlation_mode='topk_matched:1:0.0:0.0', **{key: bad})


@pytest.mark.parametrize('kind', ['s', 't'])
def test_heads_build_with_the_keys_and_validate_the_scale(kind):
    import mv2d_amd
    make = configs.roi_head_cfg_s if kind == 's' else configs.roi_head_cfg_t
    cfg = make(box_correlation=E2E_KEYS, intrins_feat_scale=0.05)
    if kind == 't':
        cfg['num_views'] = 3
    head = mv2d_amd.build_head(cfg, test_cfg=configs.TEST_CFG_RCNN)
    bc = head.box_corr_module
    assert (bc.sample_size, bc.num_depth, bc.depth_start, bc.depth_end, bc.LID) == (6, 16, 0.3, 60.0, False) and head.intrins_feat_scale == 0.05
    cfg = make()
    cfg['intrins_feat_scale'] = '0.1'
    if kind == 't':
        cfg['num_views'] = 3
    with pytest.raises(ValueError, match='intrins_feat_scale'):
        mv2d_amd.build_head(cfg, test_cfg=configs.TEST_CFG_RCNN)


def test_engine_signature_has_the_keys_at_the_shipped_values():
    import inspect
    from mv2d_amd.engine import HeadEngine
    p = inspect.signature(HeadEngine.__init__).parameters
    assert {k: p[k].default for k in ('sample_size', 'num_depth', 'corr_depth_start', 'corr_depth_end', 'corr_LID', 'intrins_feat_scale')} == \
        dict(sample_size=4, num_depth=8, corr_depth_start=0.5, corr_depth_end=70, corr_LID=True, intrins_feat_scale=0.1)


def test_new_workloads_leave_the_draws_of_the_others_alone():
    assert synthetic.WORKLOADS['corr3_s'] == ('S', 3, 1, 224, 400, 416, 12) and synthetic.WORKLOADS['corr3_t'] == ('T', 3, 1, 224, 400, 416, 12)
    assert synthetic.RIG['corr3_s'] == synthetic.RIG['corr3_t'] == (8.0, 0.35)
    a, b = synthetic.make_problem('corr3_s', seed=0), synthetic.make_problem('corr3_t', seed=0)
    assert len(a['img_metas']) == 3 and a['feat'].shape == (3, 256, 14, 26) and [len(p) for p in a['proposals']] == [12, 12, 12]
    assert all(np.array_equal(x, y) for x, y in zip(a['proposals'], b['proposals'])) and np.array_equal(a['feat'], b['feat'])
    # the rig of tests/geometry_cases.py
    ref = synthetic.make_img_metas(gc.VIEWS, gc.IMG_H, gc.IMG_W, 1, pad_w=gc.PAD_W, yaw_step_deg=gc.RIGS[0][0], baseline=gc.RIGS[0][1])
    assert all(np.array_equal(m['lidar2img'], r['lidar2img']) and m['pad_shape'] == r['pad_shape'] for m, r in zip(a['img_metas'], ref))


# ------------------------------------------------------------------------------------------------------------------------ the C entries
def test_the_ex_entries_are_declared_and_bound():
    import ctypes
    from mv2d_amd._lib import SIGNATURES
    src = open(os.path.join(ROOT, 'include', 'mv2d_hip.h')).read()
    for name, old in (('mv2d_box_correlation_ex', 'mv2d_box_correlation'), ('mv2d_frame_geometry_ex', 'mv2d_frame_geometry')):
        assert re.search(r'\bint %s\(' % name, src), name
        ret, args = SIGNATURES[name]
        ret0, args0 = SIGNATURES[old]
        assert ret is ret0 and len(args) == len(args0)
        diff = [i for i, (a, b) in enumerate(zip(args, args0)) if a is not b]
        assert len(diff) == 1 and args[diff[0]] is ctypes.c_double and args0[diff[0]] is ctypes.c_float      # depth_start alone, as a double
    from mv2d_amd import _lib
    assert _lib.ABI_VERSION == 6


# ------------------------------------------------------------------------------------------------------------------------ goldens
def test_golden_key_sets_are_the_ones_asked_for():
    assert key_sets() == [(2, 33, 0.5, 70.0, True, 20), (4, 16, 0.5, 70.0, True, 1), (3, 29, 1.0, 50.0, True, 5), (8, 64, 0.5, 70.0, True, 20),
                          (4, 8, 0.5, 35.0, True, 20), (4, 8, 0.5, 70.0, False, 20), (6, 16, 0.3, 60.0, False, 300)]
    assert [ks[0] * ks[0] * ks[1] for ks in key_sets()] == [132, 256, 261, 4096, 128, 128, 576]
    g = load_golden('box_corr_keys_kernel')
    for layout in ('r127', 'mid_empty'):
        case = gc.make_case(layout)
        for ks in key_sets():
            m = golden_match(layout, ks)
            assert m.shape == (case.R, case.V, ks[5]) and m.dtype == np.int32 and int(m.min()) == -1 and int(m.max()) < case.R
    assert len(g) == 1 + 2 * len(key_sets())


@pytest.mark.parametrize('layout', ['r127', 'mid_empty'])
def test_oracle_equals_the_reference_above_128_samples(layout):
    for ks in key_sets():
        if ks[4]:
            np.testing.assert_array_equal(oracle_match(layout, ks), golden_match(layout, ks), err_msg=str(ks))


def test_every_key_set_changes_the_lists_of_a_quarter_of_the_rois():
    """on r127, against the default keys at the same topk (the oracle's lists: the LID=True goldens equal the oracle's, see above)"""
    case = gc.make_case('r127')
    for ks in key_sets():
        base = oracle_match('r127', DEFAULT_KEYS[:4] + (True, ks[5]))
        differ = int((golden_match('r127', ks) != base).reshape(case.R, -1).any(1).sum())
        print(f'[box_corr_keys] r127 {ks}: {differ} / {case.R} RoIs with another match row than at the default keys')
        assert 4 * differ >= case.R, (ks, differ)


@pytest.mark.parametrize('name', ['corr3_s_keys', 'corr3_t_keys', 'corr3_s_scale'])
def test_end_to_end_goldens_were_recorded_off_the_default_keys(name):
    g = load_golden('box_corr_keys_' + name)
    prob = synthetic.make_problem('corr3_t' if '_t_' in name else 'corr3_s', seed=int(g['seed']))
    rois = O.bbox2roi([torch.from_numpy(p) for p in prob['proposals']])
    npv = [len(p) for p in prob['proposals']]
    R = rois.shape[0]
    K_roi, _ = O.get_box_params([torch.from_numpy(p) for p in prob['proposals']], [m['intrinsics'] for m in prob['img_metas']],
                                [m['extrinsics'] for m in prob['img_metas']])
    scale = float(g['intrins_feat_scale'])
    assert torch.equal(O.process_intrins_feat(rois, K_roi, scale, 4).clamp(-5e3, 5e3), torch.from_numpy(g['intr']))
    assert not torch.equal(O.process_intrins_feat(rois, K_roi, 0.1, 4).clamp(-5e3, 5e3), torch.from_numpy(g['intr']))
    keys = (int(g['sample_size']), int(g['num_depth']), float(g['depth_start']), float(g['depth_end']), bool(g['LID']))
    noise = load_golden('box_corr_keys_refnoise')
    assert int(noise[name + '_pairwise_ranked_diff'].max()) <= 4 and noise[name + '_topk_index'].shape == (5, 300)
    if name == 'corr3_s_scale':
        assert keys == DEFAULT_KEYS
        corr, cmask = O.gen_box_roi_correlation(rois, npv, prob['img_metas'], topk=1)
        assert np.array_equal(corr.numpy()[cmask.numpy()], g['corr'][g['corr_mask']]) and np.array_equal(cmask.numpy(), g['corr_mask'])
        return
    assert keys == tuple(E2E_KEYS[k] for k in ('sample_size', 'num_depth', 'depth_start', 'depth_end', 'LID')) and scale == 0.05
    if prob['kind'] == 'S':
        corr, cmask = O.gen_box_roi_correlation(rois, npv, prob['img_metas'], topk=1)
        rows = [sorted(corr[r][cmask[r]].tolist()) for r in range(R)]
        got = [sorted(g['corr'][r][g['corr_mask'][r]].tolist()) for r in range(R)]
        differ = sum(a != b for a, b in zip(rows, got))
    else:
        V, _, h, w = prob['feat'].shape
        ffr = O.gen_box_correlation(rois, npv, prob['img_metas'], h, w, 16, 2, 20).numpy()
        got = unpack_bits(g['feat_for_rois'], g['feat_for_rois_shape'])
        assert got.shape == ffr.shape
        differ = int((got != ffr).reshape(R, -1).any(1).sum())
    print(f'[box_corr_keys] {name}: {differ} / {R} RoIs with other keys than at the default box_correlation')
    assert differ > 0


# ------------------------------------------------------------------------------------------------------------------------ depth_start in double
def identity_case():
    """identity view-to-view transforms, the same box in two views, one depth bin: every sample lands on itself at camera depth fp32(depth_start)"""
    rois = torch.tensor([[0.0, 100.0, 60.0, 180.0, 140.0], [1.0, 100.0, 60.0, 180.0, 140.0]])
    trans = torch.eye(4, dtype=torch.float64)[None, None].repeat(2, 2, 1, 1).contiguous()
    return rois, [1, 1], (224, 416, 3), trans


@pytest.mark.parametrize('depth_start,matched', [(0.7, False), (0.9, False), (0.5, True), (0.3, True), (0.1, True)])
def test_oracle_compares_depth_start_in_double(depth_start, matched):
    """fp32(0.7) < 0.7 and fp32(0.9) < 0.9: the one depth bin lies below depth_start in double and no sample is valid; an fp32 compare would keep
    them all.  fp32(0.3) > 0.3, fp32(0.1) > 0.1 and 0.5 is exact: the two compares agree."""
    below = float(np.float32(depth_start)) < depth_start
    assert below == (not matched) and not (np.float32(depth_start) < np.float32(depth_start))
    rois, npv, shape, trans = identity_case()
    ep = O.epipolar_in_box(rois, npv, shape, trans, 1, 0.0, 0.0, 4, 1, depth_start, 70)
    assert ep == ([[(1, True)], [(0, True)]] if matched else [[], []])
