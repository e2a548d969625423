"""The PE's depth_num / depth_start / position_range on CPU: the config helpers set them, ``PE`` builds ``position_encoder.0`` for every
supported depth with the reference's parameter names, unsupported values are refused by name, the goldens of tools/gen_golden_pe_depth*.py
load with their documented keys, the host tables follow depth_start and position_range, and the size- and pitch-taking C entries are
declared and exported."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import mv2d_amd
from conftest import GOLDEN, load_golden
from mv2d_amd import _lib, calib, configs, ops, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ('mv2d_pe_fused_x3_k', 'mv2d_pe_frustum_f32_ld', 'mv2d_pe_inputs_ld')
DEPTHS = tuple(range(8, 81, 8))
RANGE_D40 = [-65.0, -65.0, -8.0, 65.0, 65.0, 8.0]
CASES = {'micro_s_d8': ('micro_s', 8), 'cfg1_s_d32': ('cfg1_s', 32), 'cfg1_t_d40': ('cfg1_t', 40), 'cfg3_t_d80': ('cfg3_t', 80)}
PE_CFG = dict(positional_encoding=dict(type='SinePositionalEncoding3D', num_feats=128, normalize=True), strides=[16], with_fpe=True)


def _pe(**kw):
    from mv2d_amd.plugin.modules import PE
    return PE(**{**PE_CFG, 'position_range': configs.POST_RANGE, 'depth_num': 64, **kw})


def test_config_helpers_set_the_three_keys():
    for fn in (configs.roi_head_cfg_s, configs.roi_head_cfg_t):
        base = fn()
        assert base['pe'] == dict(PE_CFG, strides=configs.ROI_STRIDES, position_range=configs.POST_RANGE, depth_num=64)
        assert fn(depth_num=64, depth_start=1, position_range=None) == base
        cfg = fn(depth_num=40, depth_start=2.0, position_range=RANGE_D40)
        assert cfg['pe']['depth_num'] == 40 and cfg['pe']['depth_start'] == 2.0 and cfg['pe']['position_range'] == RANGE_D40
        assert cfg['bbox_head']['bbox_coder']['post_center_range'] == configs.POST_RANGE          # the coder keeps its own range
        cfg['pe'] = base['pe']
        assert cfg == base                                                                         # nothing else moved
        assert fn()['pe']['position_range'] == configs.POST_RANGE                                  # (and no call changed the shared constant)


def test_pe_padding_rule():
    assert [ops.pe_kp(D) // 32 for D in DEPTHS] == [1, 2, 3, 3, 4, 5, 6, 6, 7, 8]
    W = torch.arange(1024 * 72, dtype=torch.float32).reshape(1024, 72, 1, 1)
    Wp = ops.pad_pe_w1a(W, 24)
    assert tuple(Wp.shape) == (1024, 96) and torch.equal(Wp[:, :72], W.flatten(1)) and not Wp[:, 72:].any()
    Wn = torch.full((1024, 96), float('nan'))
    Wn[:, :72] = W.flatten(1)
    assert torch.equal(ops.pad_pe_w1a(Wn, 24), Wp)                     # an already padded copy: its pad columns are dropped, not kept
    assert ops.pad_pe_w1a(torch.ones(1024, 96), 32).shape == (1024, 96)
    with pytest.raises(ValueError, match='3 \\* depth_num'):
        ops.pad_pe_w1a(torch.ones(1024, 192), 32)


@pytest.mark.parametrize('D', DEPTHS)
def test_pe_builds_for_every_supported_depth(D):
    pe = _pe(depth_num=D)
    assert tuple(pe.position_encoder[0].weight.shape) == (1024, 3 * D, 1, 1) and pe.depth_num == D
    ref = json.load(open(os.path.join(GOLDEN, 'pe_depth_state_keys.json')))
    for case, rec in ref.items():                                        # the reference PE's own names; its shapes at that case's depth
        want = {k: tuple(v) for k, v in rec['position_encoding'].items()}
        assert set(pe.state_dict()) == set(want)
        if rec['depth_num'] == D:
            assert {k: tuple(v.shape) for k, v in pe.state_dict().items()} == want


def test_state_keys_json_covers_the_golden_cases():
    ref = json.load(open(os.path.join(GOLDEN, 'pe_depth_state_keys.json')))
    assert set(ref) == set(CASES)
    for case, (_, D) in CASES.items():
        assert ref[case]['depth_num'] == D and ref[case]['position_encoding']['position_encoder.0.weight'] == [1024, 3 * D, 1, 1]


@pytest.mark.parametrize('cfg_fn', [configs.roi_head_cfg_s, configs.roi_head_cfg_t])
def test_head_builds_and_loads_the_depth_state(cfg_fn):
    head = mv2d_amd.build_head(cfg_fn(depth_num=24, depth_start=0.5), test_cfg=configs.TEST_CFG_RCNN)
    sd = synthetic.with_pe_depth_state(synthetic.make_head_state(seed=0), 0, 24)
    assert sd['position_encoding.position_encoder.0.weight'].shape == (1024, 72, 1, 1)
    base = synthetic.make_head_state(seed=0)
    assert set(sd) == set(base) and all(np.array_equal(sd[k], base[k]) for k in base if k != 'position_encoding.position_encoder.0.weight')
    missing, unexpected = head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not missing and not unexpected
    assert head.position_encoding.depth_num == 24 and head.position_encoding.depth_start == 0.5


@pytest.mark.parametrize('bad', [0, 4, 12, 88])
def test_depth_num_refused(bad):
    with pytest.raises(ValueError, match=r'depth_num must be a multiple of 8 in \[8, 80\]'):
        _pe(depth_num=bad)
    with pytest.raises(ValueError, match=r'depth_num must be a multiple of 8 in \[8, 80\]'):
        mv2d_amd.build_head(configs.roi_head_cfg_t(depth_num=bad), test_cfg=configs.TEST_CFG_RCNN)


@pytest.mark.parametrize('bad', [0, -1.0, 61.2, 100.0])
def test_depth_start_refused(bad):
    with pytest.raises(ValueError, match=r'depth_start must be a float with 0 < depth_start < position_range\[3\]'):
        _pe(depth_start=bad)


@pytest.mark.parametrize('bad', [[-61.2, -61.2, -10.0, -61.2, 61.2, 10.0], [-61.2, -61.2, 10.0, 61.2, 61.2, -10.0], [-61.2, -61.2, -10.0, 61.2, 61.2],
                                 [-61.2, -61.2, -10.0, 61.2, float('nan'), 10.0]])
def test_position_range_refused(bad):
    with pytest.raises(ValueError, match='position_range must be six finite floats'):
        _pe(position_range=bad)


def test_engine_argument_checks_name_the_key():
    # (HeadEngine checks its arguments before it touches the device or the weights)
    from mv2d_amd.engine import HeadEngine
    for kw, pat in ((dict(depth_num=12), 'HeadEngine: depth_num'), (dict(depth_start=0.0), 'HeadEngine: depth_start'),
                    (dict(position_range=(0, 0, 0, 1, 0, 1)), 'HeadEngine: position_range'), (dict(depth_start=70.0), 'HeadEngine: depth_start')):
        with pytest.raises(ValueError, match=pat):
            HeadEngine({}, 'T', 'cpu', **kw)


def test_goldens_load_with_documented_keys():
    rn = load_golden('pe_depth_refnoise')
    for case, (problem, D) in CASES.items():
        g = load_golden('pe_depth_' + case)
        kind = synthetic.WORKLOADS[problem][0]
        assert int(g['depth_num']) == D
        R = g['intr'].shape[0]
        assert g['intr'].shape == (R, 16) and g['cls'].shape[0] == 6 and g['cls'].size == 6 * R * 10 and g['reg'].shape == g['cls'].shape
        assert g['center_pred'].shape == (R, 3) and g['xyz'].shape == (R, 3)
        n = len(g['labels'])
        assert g['boxes'].shape == (n, 9) and g['scores'].shape == (n,) and g['topk_index'].shape == (n,) and g['topk_scores'].shape == (n,)
        assert ('feat_for_rois' in g and 'key_padding' in g) if kind == 'T' else ('corr' in g and 'corr_mask' in g)
        key = case + '_s0'
        assert int(rn[key + '_pairwise_ranked_diff'].max()) <= 4           # the project's NOISE_MAX
        assert rn[key + '_topk_index'].shape == (5, n)
        assert os.path.getsize(os.path.join(GOLDEN, f'pe_depth_{case}.npz')) < 200 * 1024
    g = load_golden('pe_depth_cfg1_t_d40')
    assert float(g['depth_start']) == 2.0 and g['position_range'].tolist() == RANGE_D40
    g = load_golden('pe_depth_micro_s_d8')
    assert float(g['depth_start']) == 1.0 and g['position_range'].tolist() == configs.POST_RANGE
    assert g['pe_rows'].shape == (len(g['pe_positions']), 256) and int(g['pe_positions'].max()) < 2 * 8 * 12
    t = load_golden('pe_depth_train_d32')
    for name in ('train_micro_t', 'train_micro_s'):
        names = [str(n) for n in t[name + '.grad_names']]
        assert len(names) == 232 and 'position_encoding.position_encoder.0.weight' in names
        assert t[name + '.grad_norm'].shape == (232,) and t[name + '.grad_proj'].shape == (232,)
        assert t[name + '.match'].shape[0] == 6 and t[name + '.cls'].shape[0] == 6
        assert any(k.startswith(name + '.loss.') for k in t)
    assert any(k.startswith('train_micro_t.loss.') and 'dn_loss' in k for k in t)


def test_host_tables_follow_depth_start_and_position_range():
    """calib.shape_tables at depth_start = 2.0: coords_d as MU/pe.py:96-100 defines it, and the frustum rows rebuilt from the host tables equal
    oracle.mv2d_oracle.pe_frustum_input(depth_num=40, depth_start=2.0, position_range=...)."""
    from oracle import mv2d_oracle as O
    prob = synthetic.make_problem('micro_t', seed=0)
    metas = prob['img_metas']
    V, _, h, w = prob['feat'].shape
    D = 40
    sht = calib.shape_tables(calib.meta_shapes(metas), h, w, depth_num=D, depth_start=2.0, position_range=tuple(RANGE_D40))
    idx = torch.arange(D).double()
    want_d = 2.0 + (65.0 - 2.0) / (D * (1 + D)) * idx * (idx + 1)
    assert sht['coords_d'].dtype == torch.float64 and torch.equal(sht['coords_d'], want_d)
    assert float(sht['coords_d'][0]) == 2.0 and float(sht['coords_d'][-1]) < 65.0
    assert not torch.equal(sht['coords_d'], calib.shape_tables(calib.meta_shapes(metas), h, w, depth_num=D, position_range=tuple(RANGE_D40))['coords_d'])
    ft = calib.frame_tables(metas, h, w, depth_num=D, depth_start=2.0, position_range=tuple(RANGE_D40))
    assert torch.equal(ft['coords_d'], sht['coords_d'])
    M = ft['img2lidar'].view(V, 4, 4)
    cw, ch, cd = ft['coords_w'], ft['coords_h'], ft['coords_d']
    dm = cd.clamp_min(1e-3)
    pts = torch.stack([cw[None, :, None] * dm[None, None, :] * torch.ones(h, 1, 1, dtype=torch.float64),
                       ch[:, None, None] * dm[None, None, :] * torch.ones(1, w, 1, dtype=torch.float64),
                       cd[None, None, :] * torch.ones(h, w, 1, dtype=torch.float64), torch.ones(h, w, D, dtype=torch.float64)], -1)      # [h,w,D,4]
    c3 = torch.einsum('vij,hwdj->vhwdi', M, pts)[..., :3]
    lo, hi = torch.tensor(RANGE_D40[:3], dtype=torch.float64), torch.tensor(RANGE_D40[3:], dtype=torch.float64)
    nrm = ((c3 - lo) / (hi - lo)).clamp(0, 1)
    rows = torch.log(nrm.clamp_min(1e-5) / (1 - nrm).clamp_min(1e-5)).float().reshape(V, h, w, 3 * D)
    ref = O.pe_frustum_input(metas, h, w, depth_num=D, depth_start=2.0, position_range=RANGE_D40).permute(0, 2, 3, 1)
    d = (rows - ref).abs()
    assert float((d / ref.abs().clamp_min(1e-3)).max()) < 3e-7 and int((d > 0).sum()) <= max(1, d.numel() // 1000)


def test_new_entries_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    lib = _lib.load()
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mv2d_hip.h')).read(), flags=re.S)
    for n in NEW_ENTRIES:
        assert re.search(r'\b' + n + r'\s*\(', hdr), n
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert lib.mv2d_abi_version() == 6
    # argument checks run before any device call: sizes the kernels have no instance for are errors, not silent reads past a row
    assert lib.mv2d_pe_fused_x3_k(*([None] * 4), 4, *([None] * 13), 1, *([None] * 5), 0, 0, None, 0, 96 + 8, None) == -1
    assert b'Kp' in lib.mv2d_last_error()
    assert lib.mv2d_pe_fused_x3_k(*([None] * 4), 4, *([None] * 13), 1, *([None] * 5), 0, 0, None, 0, 288, None) == -1
    one = (ctypes.c_double * 8)()                                       # any non-null pointer: the size checks come first
    assert lib.mv2d_pe_frustum_f32_ld(one, one, 4, one, one, one, one, one, 1, 2, 2, 40, one, 96, None) == -1 and b'ld' in lib.mv2d_last_error()
    assert lib.mv2d_pe_inputs_ld(*([one] * 2), 4, *([one] * 13), 1, 2, 2, 40, one, 0, 100, None) == -1 and b'ld' in lib.mv2d_last_error()
