"""Class counts other than nuScenes' 10 on CPU: the reference config key ``num_classes`` (head and coder) builds S and T heads whose
state dict differs from the 10-class one only in the class output layers; out-of-range counts and a coder / head mismatch are refused;
the synthetic weights keep their 10-class stream."""
import numpy as np
import pytest
import torch

import mv2d_amd
from mv2d_amd import configs, synthetic


def _shapes(head):
    return {k: tuple(v.shape) for k, v in head.state_dict().items()}


@pytest.mark.parametrize('cfg_fn', [configs.roi_head_cfg_s, configs.roi_head_cfg_t])
@pytest.mark.parametrize('N', [1, 3, 26, 64])
def test_head_state_dict_with_num_classes(cfg_fn, N):
    base = _shapes(mv2d_amd.build_head(cfg_fn(), test_cfg=configs.TEST_CFG_RCNN))
    head = mv2d_amd.build_head(cfg_fn(num_classes=N), test_cfg=configs.TEST_CFG_RCNN)
    assert head.num_classes == N and head.bbox_head.bbox_coder.num_classes == N
    got = _shapes(head)
    assert set(got) == set(base)
    L = head.bbox_head.num_pred
    cls_out = {f'bbox_head.cls_branches.{l}.6.{p}' for l in range(L) for p in ('weight', 'bias')}
    for k, shp in got.items():
        if k in cls_out:
            assert shp == ((N, 256) if k.endswith('weight') else (N,)), (k, shp)
        else:
            assert shp == base[k], (k, shp, base[k])
    # the synthetic weights of that class count load strictly
    sd = {k: torch.from_numpy(v) for k, v in synthetic.make_head_state(seed=0, num_classes=N).items()}
    missing, unexpected = head.load_state_dict(sd, strict=True)
    assert not missing and not unexpected


@pytest.mark.parametrize('N', [0, 65])
def test_num_classes_out_of_range(N):
    with pytest.raises(ValueError, match='64'):
        mv2d_amd.build_head(configs.roi_head_cfg_s(num_classes=N), test_cfg=configs.TEST_CFG_RCNN)


def test_coder_head_mismatch():
    cfg = configs.roi_head_cfg_s(num_classes=3)
    cfg['bbox_head']['bbox_coder']['num_classes'] = 10
    with pytest.raises(ValueError, match='bbox_coder'):
        mv2d_amd.build_head(cfg, test_cfg=configs.TEST_CFG_RCNN)


def test_default_configs_unchanged():
    for fn in (configs.roi_head_cfg_s, configs.roi_head_cfg_t):
        assert fn() == fn(num_classes=10)
        assert fn()['bbox_head']['num_classes'] == 10 and fn()['bbox_head']['bbox_coder']['num_classes'] == 10


def test_make_head_state_default_stream():
    a = synthetic.make_head_state(seed=0, num_classes=10)
    b = synthetic.make_head_state(seed=0)
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    c = synthetic.make_head_state(seed=0, num_classes=3)
    assert c['bbox_head.cls_branches.0.6.weight'].shape == (3, 256)
    # everything drawn before the class output layers is the same stream
    np.testing.assert_array_equal(c['bbox_head.cls_branches.0.4.weight'], b['bbox_head.cls_branches.0.4.weight'])
