"""RoI sizes other than 7 on CPU: ``configs.roi_head_cfg_s/t(roi_size=s)`` set the RoI extractor's RoIAlign and the query generator together
and build S and T heads whose state dict is the 7x7 one (no weight shape depends on s); non-square, out-of-range and mismatched sizes are
refused; the size-taking C entries are declared and exported."""
import os
import re

import pytest
import torch

import mv2d_amd
from mv2d_amd import _lib, configs, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ('mv2d_roi_align_s', 'mv2d_roi_align_bwd_s', 'mv2d_csr_from_corr_s', 'mv2d_roi_positions_csr_s', 'mv2d_qg_conv_pool_s',
               'mv2d_qg_conv_pool_x3_s', 'mv2d_im2col3x3_s', 'mv2d_col2im3x3_s')


def _shapes(head):
    return {k: tuple(v.shape) for k, v in head.state_dict().items()}


@pytest.mark.parametrize('cfg_fn', [configs.roi_head_cfg_s, configs.roi_head_cfg_t])
@pytest.mark.parametrize('s', [1, 5, 9, 14])
def test_head_builds_with_roi_size(cfg_fn, s):
    cfg = cfg_fn(roi_size=s)
    assert cfg['bbox_roi_extractor']['roi_layer']['output_size'] == s and cfg['query_generator']['roi_feat_size'] == s
    head = mv2d_amd.build_head(cfg, test_cfg=configs.TEST_CFG_RCNN)
    assert head.roi_cells == s and head.roi_size == [s, s]
    assert head.bbox_roi_extractor.roi_size == s and head.query_generator.roi_feat_size == s
    assert _shapes(head) == _shapes(mv2d_amd.build_head(cfg_fn(), test_cfg=configs.TEST_CFG_RCNN))


def test_state_dict_made_at_7_loads_at_5():
    sd = {k: torch.from_numpy(v) for k, v in synthetic.make_head_state(seed=0).items()}
    for fn in (configs.roi_head_cfg_s, configs.roi_head_cfg_t):
        head = mv2d_amd.build_head(fn(roi_size=5), test_cfg=configs.TEST_CFG_RCNN)
        missing, unexpected = head.load_state_dict(sd, strict=True)
        assert not missing and not unexpected


def test_pair_sizes_accepted():
    cfg = configs.roi_head_cfg_s(roi_size=(5, 5))
    assert mv2d_amd.build_head(cfg, test_cfg=configs.TEST_CFG_RCNN).roi_cells == 5


@pytest.mark.parametrize('bad', [0, 15, (5, 7), 7.5, (5, 5, 5)])
def test_roi_size_out_of_range(bad):
    with pytest.raises(ValueError, match=r'\[1, 14\]|1 <= s <= 14'):
        mv2d_amd.build_head(configs.roi_head_cfg_s(roi_size=bad), test_cfg=configs.TEST_CFG_RCNN)


def test_extractor_query_generator_mismatch():
    cfg = configs.roi_head_cfg_t(roi_size=5)
    cfg['query_generator']['roi_feat_size'] = 7
    with pytest.raises(ValueError, match='must agree'):
        mv2d_amd.build_head(cfg, test_cfg=configs.TEST_CFG_RCNN)


def test_default_configs_unchanged():
    for fn in (configs.roi_head_cfg_s, configs.roi_head_cfg_t):
        assert fn() == fn(roi_size=7)
        assert fn()['bbox_roi_extractor']['roi_layer']['output_size'] == 7 and fn()['query_generator']['roi_feat_size'] == 7


def test_engine_refuses_bad_roi_size():
    from mv2d_amd.engine import HeadEngine
    for bad in (0, 15, 5.5):
        with pytest.raises(ValueError, match=r'\[1, 14\]'):
            HeadEngine({}, 'S', 'cpu', roi_size=bad)


def test_new_entries_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'mv2d_hip.h')).read()
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES, name
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\);', header)
        assert m, name
        assert len([a for a in m.group(1).split(',') if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
        assert m.group(1).rstrip().endswith('int roi_size, void* stream'), name
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name


def test_golden_files_shapes():
    """tests/golden/roi_size_*.npz (tools/gen_golden_roi_size*.py): the four inference cases and the training record at s = 5."""
    import numpy as np
    gd = os.path.join(ROOT, 'tests', 'golden')
    rn = np.load(os.path.join(gd, 'roi_size_refnoise.npz'))
    for name, s, R in (('cfg2_s', 5, 300), ('cfg3_t', 9, 300), ('nc6_s', 14, 84), ('cfg1_s', 1, 50)):
        g = np.load(os.path.join(gd, f'roi_size_{name}_s{s}.npz'))
        assert g['cls'].shape[0] == 6 and g['cls'].size == 6 * R * 10 and g['reg'].size == 6 * R * 10
        assert g['intr'].shape == (R, 16) and g['K_roi'].shape == (R, 4, 4)
        n = len(g['labels'])
        assert g['topk_index'].shape == (n,) and g['topk_scores'].shape == (n,) and g['boxes'].shape == (n, 9)
        if name.endswith('_s'):
            assert g['corr'].shape == g['corr_mask'].shape and g['corr'].shape[0] == R
        else:
            assert tuple(g['feat_for_rois_shape'])[0] == R
        key = f'{name}_s{s}_s0'
        assert rn[key + '_topk_index'].shape == (5, n) and rn[key + '_pairwise_ranked_diff'].shape == (5, 5)
    t = np.load(os.path.join(gd, 'roi_size_train_s5.npz'))
    for name in ('train_cfg1_s', 'train_cfg1_t'):
        assert len(t[name + '.grad_names']) == 232 and t[name + '.grad_norm'].shape == (232,) and t[name + '.grad_proj'].shape == (232,)
        assert t[name + '.match'].shape[0] == 6 and t[name + '.cls'].shape[0] == 6
        assert any(k.startswith(name + '.loss.') for k in t.files)
        assert t[name + '.dfeat_view_norms'].ndim == 1
    for f in os.listdir(gd):
        if f.startswith('roi_size_'):
            assert os.path.getsize(os.path.join(gd, f)) < 1 << 20, f
