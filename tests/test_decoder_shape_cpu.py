"""The decoder's shape keys on CPU (``bbox_head.transformer.decoder.num_layers`` and ``...transformerlayers.feedforward_channels``): the config
helpers set the two keys and their defaults give today's dicts, ops.check_decoder_shape is the one accepted set (in the helpers, the engine and the
synthetic state), ``synthetic.with_decoder_shape_state`` keeps every tensor it does not own bit for bit, the plugin heads built from the case configs
have the reference module's parameter names and shapes (tests/golden/decoder_shape_state_keys.json, tools/gen_golden_decoder_shape.py) and load the
case state strictly, and the golden files have the shapes their ``num_layers`` implies."""
import json
import os

import numpy as np
import pytest
import torch

import mv2d_amd
from conftest import GOLDEN, load_golden
from mv2d_amd import configs, ops, synthetic

KEYS = json.load(open(os.path.join(GOLDEN, 'decoder_shape_state_keys.json')))
# (case, problem, num_layers, feedforward_channels): the table of the generator
CASES = [('micro_s_l3', 'micro_s', 3, 2048), ('micro_t_l2_f448', 'micro_t', 2, 448), ('cfg1_t_l8_f576', 'cfg1_t', 8, 576),
         ('cfg1_s_l1_f4096', 'cfg1_s', 1, 4096), ('cfg1_s_f1024', 'cfg1_s', 6, 1024)]
DEC = 'bbox_head.transformer.decoder.'
OWNED = (DEC + 'layers.', 'bbox_head.cls_branches.', 'bbox_head.reg_branches.')
BAD_LAYERS = (0, 9, True, 2.0, '3', None, -1)
BAD_WIDTHS = (0, 96, 4160, '1024', True, 1024.0, None, -64)


def _dec(cfg):
    return cfg['bbox_head']['transformer']['decoder']


def test_config_helpers_set_the_two_keys_and_default_to_todays_dict():
    for fn in (configs.roi_head_cfg_s, configs.roi_head_cfg_t):
        base = fn()
        assert fn(num_layers=6, feedforward_channels=2048) == base
        assert _dec(base)['num_layers'] == 6 and _dec(base)['transformerlayers']['feedforward_channels'] == 2048
        for L, F in ((3, 2048), (6, 1024), (1, 64), (8, 4096), (2, 448)):
            cfg = fn(num_layers=L, feedforward_channels=F)
            assert _dec(cfg)['num_layers'] == L and _dec(cfg)['transformerlayers']['feedforward_channels'] == F
            # nothing else moves
            _dec(cfg)['num_layers'], _dec(cfg)['transformerlayers']['feedforward_channels'] = 6, 2048
            assert cfg == base
        assert fn() == base
        # together with another key
        cfg = fn(num_layers=3, num_reg_fcs=1, num_classes=3)
        assert _dec(cfg)['num_layers'] == 3 and cfg['bbox_head']['num_reg_fcs'] == 1 and cfg['bbox_head']['num_classes'] == 3


def test_check_accepts_and_refuses():
    for L in range(1, 9):
        assert ops.check_decoder_shape(L, 2048, 'x') == (L, 2048)
    for F in range(64, 4097, 64):
        assert ops.check_decoder_shape(6, F, 'x') == (6, F)
    assert ops.check_decoder_shape(np.int64(3), np.int32(448), 'x') == (3, 448)
    for v in BAD_LAYERS:
        with pytest.raises(ValueError, match='who: num_layers'):
            ops.check_decoder_shape(v, 2048, 'who')
    for v in BAD_WIDTHS:
        with pytest.raises(ValueError, match='who: feedforward_channels'):
            ops.check_decoder_shape(6, v, 'who')
    assert [ops.ffn_slabs(F) for F in (64, 448, 512, 576, 1024, 1984, 2048, 4096)] == [1, 1, 1, 2, 2, 4, 4, 8]


@pytest.mark.parametrize('v', [0, 9, True, 2.0])
def test_every_entry_refuses_a_bad_num_layers(v):
    from mv2d_amd.engine import HeadEngine
    for fn in (configs.roi_head_cfg_s, configs.roi_head_cfg_t):
        with pytest.raises(ValueError, match='num_layers'):
            fn(num_layers=v)
    with pytest.raises(ValueError, match='HeadEngine: num_layers'):           # (HeadEngine checks its arguments before it touches the device or the weights)
        HeadEngine({}, 'S', 'cpu', num_layers=v)
    with pytest.raises(ValueError, match='num_layers'):
        synthetic.with_decoder_shape_state({}, 0, v, 2048)


@pytest.mark.parametrize('v', [0, 96, 4160, '1024'])
def test_every_entry_refuses_a_bad_feedforward_channels(v):
    from mv2d_amd.engine import HeadEngine
    for fn in (configs.roi_head_cfg_s, configs.roi_head_cfg_t):
        with pytest.raises(ValueError, match='feedforward_channels'):
            fn(feedforward_channels=v)
    with pytest.raises(ValueError, match='HeadEngine: feedforward_channels'):
        HeadEngine({}, 'T', 'cpu', feedforward_channels=v)
    with pytest.raises(ValueError, match='feedforward_channels'):
        synthetic.with_decoder_shape_state({}, 0, 6, v)


def test_engine_state_check_names_the_key():
    """HeadEngine.check_decoder_shape, as load_state calls it first: a layer count or an FFN width other than the engine's is a ValueError."""
    from mv2d_amd.engine import HeadEngine
    base = synthetic.make_head_state(seed=0)
    HeadEngine.check_decoder_shape(base, 6, 2048)
    for n in (4, 8):
        with pytest.raises(ValueError, match=rf'num_layers=6, the state dict holds {n} decoder layers'):
            HeadEngine.check_decoder_shape(synthetic.with_decoder_shape_state(base, 0, n, 2048), 6, 2048)
    narrow = synthetic.with_decoder_shape_state(base, 0, 6, 1024)
    with pytest.raises(ValueError, match=r'feedforward_channels=2048 expects .*layers\.0\.ffns\.0\.layers\.0\.0\.weight to be \(2048, 256\).*\(1024, 256\)'):
        HeadEngine.check_decoder_shape(narrow, 6, 2048)
    HeadEngine.check_decoder_shape(narrow, 6, 1024)
    mixed = dict(narrow)
    mixed[DEC + 'layers.4.ffns.0.layers.1.weight'] = base[DEC + 'layers.4.ffns.0.layers.1.weight']
    with pytest.raises(ValueError, match=r'feedforward_channels=1024 expects .*layers\.4\.ffns\.0\.layers\.1\.weight to be \(256, 1024\)'):
        HeadEngine.check_decoder_shape(mixed, 6, 1024)


def test_with_decoder_shape_state_keeps_what_it_does_not_own():
    base = synthetic.make_head_state(seed=0)
    same = synthetic.with_decoder_shape_state(base, 0, 6, 2048)
    assert list(same) == list(base) and all(np.array_equal(same[k], base[k]) for k in base)         # the shipped shape: every tensor, bit for bit
    for _, _, L, F in CASES + [('', '', 7, 64)]:
        sd = synthetic.with_decoder_shape_state(base, 0, L, F)
        for k, v in sd.items():
            assert v.dtype == np.float32, k
            if not k.startswith(OWNED):
                assert np.array_equal(v, base[k]), k                                                  # every non-decoder tensor
        assert [k for k in base if not k.startswith(OWNED)] == [k for k in sd if not k.startswith(OWNED)]
        for prefix in OWNED:
            assert {int(k[len(prefix):].split('.')[0]) for k in sd if k.startswith(prefix)} == set(range(L))
        for l in range(L):
            p = f'{DEC}layers.{l}.'
            assert sd[p + 'ffns.0.layers.0.0.weight'].shape == (F, 256) and sd[p + 'ffns.0.layers.0.0.bias'].shape == (F,)
            assert sd[p + 'ffns.0.layers.1.weight'].shape == (256, F) and sd[p + 'ffns.0.layers.1.bias'].shape == (256,)
            for k in (k for k in sd if k.startswith((p,) + tuple(f'{h}{l}.' for h in OWNED[1:]))):
                if l < 6 and (F == 2048 or '.ffns.' not in k):
                    assert np.array_equal(sd[k], base[k]), k                                          # a kept layer keeps everything but a redrawn FFN
                else:
                    if '.ffns.' not in k:                                                             # a new layer: layer 0's names and shapes
                        assert sd[k].shape == base[k.replace(f'.{l}.', '.0.', 1)].shape, k
                    assert np.isfinite(sd[k]).all() and float(np.abs(sd[k]).max()) > 0
        # repeatable, and another seed draws other tensors
        again = synthetic.with_decoder_shape_state(base, 0, L, F)
        assert all(np.array_equal(sd[k], again[k]) for k in sd)
        if F != 2048:
            other = synthetic.with_decoder_shape_state(base, 1, L, F)
            assert not np.array_equal(sd[DEC + 'layers.0.ffns.0.layers.0.0.weight'], other[DEC + 'layers.0.ffns.0.layers.0.0.weight'])
    assert synthetic.make_head_state(seed=0).keys() == base.keys() and all(np.array_equal(synthetic.make_head_state(seed=0)[k], base[k]) for k in base)


def _head(kind, L, F, train_cfg=None):
    cfg = (configs.roi_head_cfg_s if kind == 'S' else configs.roi_head_cfg_t)(num_layers=L, feedforward_channels=F)
    if kind == 'T':
        cfg['num_views'] = 2
    return mv2d_amd.build_head(cfg, train_cfg=train_cfg, test_cfg=configs.TEST_CFG_RCNN)


@pytest.mark.parametrize('case,problem,L,F', CASES)
def test_plugin_head_builds_the_reference_names_and_shapes(case, problem, L, F):
    rec = KEYS[case]
    assert (rec['problem'], rec['num_layers'], rec['feedforward_channels'], rec['kind']) == (problem, L, F, synthetic.WORKLOADS[problem][0])
    head = _head(rec['kind'], L, F)
    own = {k: list(v.shape) for k, v in head.state_dict().items() if k.startswith(OWNED + (DEC,))}
    assert own == rec['params']
    assert head.decoder_shape() == (L, F)
    sd = synthetic.with_decoder_shape_state(synthetic.make_head_state(seed=0), rec['seed'], L, F)
    missing, unexpected = head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not missing and not unexpected


def test_plugin_head_refuses_disagreeing_layers_and_short_stage_loss_weights():
    head = _head('S', 2, 448)
    head.bbox_head.transformer.decoder.layers[1].ffns[0].layers[0][0] = torch.nn.Linear(256, 512)
    with pytest.raises(ValueError, match='feedforward_channels disagree'):
        head.decoder_shape()
    with pytest.raises(ValueError, match=r'stage_loss_weights has 6 entries.*num_layers = 8'):
        _head('T', 8, 2048, train_cfg=configs.TRAIN_CFG_RCNN)
    _head('S', 3, 448, train_cfg=dict(configs.TRAIN_CFG_RCNN, stage_loss_weights=[0.1] * 3))
    _head('S', 3, 448, train_cfg=configs.TRAIN_CFG_RCNN)                      # a longer list is fine, as in the reference


def test_goldens_have_the_shapes_their_num_layers_implies():
    rn = load_golden('decoder_shape_refnoise')
    assert set(KEYS) == {c[0] for c in CASES}
    for case, problem, L, F in CASES:
        g = load_golden('decoder_shape_' + case)
        assert int(g['num_layers']) == L and int(g['feedforward_channels']) == F
        R = g['xyz'].shape[0]
        assert g['center_pred'].shape == (R, 3) and g['cls'].shape[0] == L and g['cls'].size == L * R * 10 and g['reg'].size == L * R * 10
        n = len(g['labels'])
        assert g['boxes'].shape == (n, 9) and g['topk_index'].shape == (n,) and rn[case + '_s0_topk_index'].shape == (5, n)
        assert int(rn[case + '_s0_pairwise_ranked_diff'].max()) <= 4           # the project's NOISE_MAX
        assert os.path.getsize(os.path.join(GOLDEN, f'decoder_shape_{case}.npz')) < 200 * 1024
    t = load_golden('decoder_shape_train')
    name = 'train_micro_s'
    assert int(t['num_layers']) == 3 and int(t['feedforward_channels']) == 448
    assert t[name + '.match'].shape[0] == 3 and t[name + '.cls'].shape[0] == 3
    assert {k[len(name) + 6:] for k in t if k.startswith(name + '.loss.')} >= {f'l{i}.loss_{x}' for i in range(3) for x in ('cls', 'bbox')}
    assert not any(k.startswith(name + '.loss.l3.') for k in t)
    names = [str(n) for n in t[name + '.grad_names']]
    assert f'{DEC}layers.2.ffns.0.layers.0.0.weight' in names and f'{DEC}layers.3.ffns.0.layers.0.0.weight' not in names
