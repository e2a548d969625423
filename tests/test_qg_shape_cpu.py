"""The query generator's shape keys on CPU (mv2d_amd/qg_shape.py): the plugin module builds the reference module's parameter names and shapes for
every golden case of tools/gen_golden_qg_shape.py (tests/golden/qg_shape_state_keys.json) and today's for the default, every refused setting raises
``ValueError`` naming its key -- in the module constructor and in the engine --, a state dict of another shape is refused by parameter name, the
flatten permutation round-trips against ``torch.flatten(1)``, the goldens load with their documented keys and the new C entries are declared."""
import json
import os
import re

import numpy as np
import pytest
import torch

import mv2d_amd
from conftest import GOLDEN, load_golden
from mv2d_amd import _lib, configs, qg_shape, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ('mv2d_qg_conv_cells', 'mv2d_qg_conv_cells_x3', 'mv2d_avgpool_cells')
KEYS = json.load(open(os.path.join(GOLDEN, 'qg_shape_state_keys.json')))
CASES = ('micro_s_c2', 'cfg1_t_c0_f2', 'cfg1_s_flat3', 'cfg1_t_enc')
DEFAULT_PARAMS = {'shared_convs.0.conv.weight': (256, 256, 3, 3), 'shared_convs.0.conv.bias': (256,), 'shared_fcs.0.weight': (1024, 256),
                  'shared_fcs.0.bias': (1024,), 'extra_enc.0.weight': (512, 1040), 'extra_enc.0.bias': (512,), 'extra_enc.2.weight': (256, 512),
                  'extra_enc.2.bias': (256,), 'fc_center.weight': (3, 256), 'fc_center.bias': (3,)}
# (setting, the key the error has to name)
REFUSED = [(dict(num_shared_fcs=0), 'num_shared_fcs'), (dict(num_shared_fcs=4), 'num_shared_fcs'), (dict(num_shared_convs=4), 'num_shared_convs'),
           (dict(num_shared_convs=-1), 'num_shared_convs'), (dict(num_center_fcs=3), 'num_center_fcs'), (dict(num_center_convs=1), 'num_center_convs'),
           (dict(with_cls=True), 'with_cls'), (dict(with_size=True), 'with_size'), (dict(with_heading=True), 'with_heading'),
           (dict(with_attr=True), 'with_attr'), (dict(num_cls_fcs=1), 'num_cls_fcs'), (dict(num_attr_convs=2), 'num_attr_convs'),
           (dict(conv_out_channels=128), 'conv_out_channels'), (dict(in_channels=512), 'in_channels'),
           (dict(fc_out_channels=1000), 'fc_out_channels'), (dict(fc_out_channels=8192), 'fc_out_channels'), (dict(fc_out_channels=0), 'fc_out_channels'),
           (dict(extra_encoding=dict(num_layers=2, feat_channels=[512, 250], features=[])), r'extra_encoding\.feat_channels'),
           (dict(extra_encoding=dict(num_layers=3, feat_channels=[512, 256], features=[])), r'extra_encoding\.feat_channels'),
           (dict(extra_encoding=dict(num_layers=0, feat_channels=[], features=[])), r'extra_encoding\.num_layers'),
           (dict(extra_encoding=dict(num_layers=4, feat_channels=64, features=[])), r'extra_encoding\.num_layers'),
           (dict(extra_encoding=dict(num_layers=1, feat_channels=64, features=[dict(type='extrinsic', in_channels=16)])), r'extra_encoding\.features'),
           (dict(extra_encoding=dict(num_layers=1, feat_channels=64, features=[dict(type='intrinsic', in_channels=9)])), r'extra_encoding\.features'),
           (dict(with_avg_pool=None), 'with_avg_pool'), (dict(norm_cfg=dict(type='BN')), 'norm_cfg')]


def _cfg(kind, keys=None, roi_size=7):
    cfg = (configs.roi_head_cfg_s if kind == 'S' else configs.roi_head_cfg_t)(query_generator=keys, roi_size=roi_size)
    if kind == 'T':
        cfg['num_views'] = 6
    return cfg


def _head(kind, keys=None, roi_size=7):
    return mv2d_amd.build_head(_cfg(kind, keys, roi_size), test_cfg=configs.TEST_CFG_RCNN)


def _shapes(mod):
    return {k: tuple(v.shape) for k, v in mod.state_dict().items()}


def test_config_helpers_lay_the_keys_over_the_shipped_subtree():
    for fn in (configs.roi_head_cfg_s, configs.roi_head_cfg_t):
        base = fn()
        assert fn(query_generator=None) == base and fn(query_generator={}) == base
        ee = dict(num_layers=1, feat_channels=64, features=[])
        cfg = fn(query_generator=dict(num_shared_convs=2, with_avg_pool=False, extra_encoding=ee), roi_size=3)
        qg = cfg['query_generator']
        assert qg['num_shared_convs'] == 2 and qg['with_avg_pool'] is False and qg['extra_encoding'] == ee and qg['roi_feat_size'] == 3
        assert qg['num_shared_fcs'] == 1 and qg['fc_out_channels'] == 1024
        ee['features'].append(1)                                               # the config holds its own copy
        assert cfg['query_generator']['extra_encoding']['features'] == []
        assert fn() == base


def test_state_keys_json_covers_the_golden_cases():
    assert set(KEYS) == set(CASES)
    for rec in KEYS.values():
        shape = qg_shape.parse(rec['query_generator'])
        assert {k: list(v) for k, v in shape.param_shapes(rec['roi_size']).items()} == rec['params']


@pytest.mark.parametrize('case', CASES)
def test_module_builds_the_reference_names_and_shapes(case):
    rec = KEYS[case]
    head = _head(rec['kind'], rec['query_generator'], rec['roi_size'])
    assert _shapes(head.query_generator) == {k: tuple(v) for k, v in rec['params'].items()}
    sd = synthetic.with_qg_shape_state(synthetic.make_head_state(seed=0), 0, rec['query_generator'], rec['roi_size'])
    base = synthetic.make_head_state(seed=0)
    assert all(np.array_equal(sd[k], base[k]) for k in base if not k.startswith('query_generator.'))      # its own stream of draws
    missing, unexpected = head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not missing and not unexpected


def test_default_module_builds_todays_parameters():
    from mv2d_amd.plugin.modules import QueryGenerator
    for head in (_head('S'), _head('T')):
        assert _shapes(head.query_generator) == DEFAULT_PARAMS and list(head.query_generator.state_dict()) == list(DEFAULT_PARAMS)
        assert head.query_generator.shape.is_default
        head.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_head_state(seed=0).items()}, strict=True)
    # the default shape written out explicitly is the default shape
    explicit = dict(with_avg_pool=True, num_shared_convs=1, num_shared_fcs=1, num_center_fcs=0, num_center_convs=0, fc_out_channels=1024,
                    conv_out_channels=256, in_channels=256, extra_encoding=dict(num_layers=2, feat_channels=[512, 256], features=[dict(type='intrinsic', in_channels=16)]))
    assert qg_shape.parse(explicit) == qg_shape.parse(None) == qg_shape.DEFAULT and qg_shape.DEFAULT.is_default
    assert _shapes(QueryGenerator(**explicit)) == DEFAULT_PARAMS
    assert qg_shape.DEFAULT.param_shapes(7) == DEFAULT_PARAMS
    # one int repeated num_layers times, as the reference takes it
    assert qg_shape.parse(dict(extra_encoding=dict(num_layers=3, feat_channels=128, features=[]))).enc == (128, 128, 128)


@pytest.mark.parametrize('keys,pat', REFUSED, ids=[next(iter(k)) + str(i) for i, (k, _) in enumerate(REFUSED)])
def test_refused_settings_name_their_key(keys, pat):
    from mv2d_amd.engine import HeadEngine
    from mv2d_amd.plugin.modules import QueryGenerator
    with pytest.raises(ValueError, match='QueryGenerator: .*' + pat):
        QueryGenerator(**keys)
    with pytest.raises(ValueError, match='QueryGenerator: .*' + pat):
        _head('T', keys)
    with pytest.raises(ValueError, match='HeadEngine: .*' + pat):           # (HeadEngine checks its arguments before it touches the device or the weights)
        HeadEngine({}, 'S', 'cpu', query_generator=keys)


@pytest.mark.parametrize('keys,pat', [(dict(num_shared_convs=None), 'num_shared_convs'), (dict(num_shared_fcs='abc'), 'num_shared_fcs'),
                                      (dict(fc_out_channels=None), 'fc_out_channels'), (dict(num_center_fcs=1.0), 'num_center_fcs'),
                                      (dict(extra_encoding=dict(feat_channels=[64], features=[])), r'extra_encoding\.num_layers is missing'),
                                      (dict(extra_encoding=dict(num_layers=1, features=[])), r'extra_encoding\.feat_channels is missing'),
                                      (dict(extra_encoding=dict(num_layers=1, feat_channels='64', features=[])), r'extra_encoding\.feat_channels')])
def test_values_of_another_type_are_refused_with_a_value_error(keys, pat):
    with pytest.raises(ValueError, match='QueryGenerator: ' + pat):
        qg_shape.parse(keys)


def test_partial_non_strict_load_still_reports_missing_keys():
    """Missing and unexpected keys stay with torch's strict handling, as before: a checkpoint without the query generator (a 2-D pretrained
    detector), or without one of its parameters, loads non-strictly and reports what it lacks; strictly it is torch's RuntimeError."""
    base = {k: torch.from_numpy(v) for k, v in synthetic.make_head_state(seed=0).items()}
    for kind, keys in (('S', None), ('T', None), ('T', KEYS['cfg1_t_c0_f2']['query_generator'])):
        head = _head(kind, keys)
        own = ['query_generator.' + k for k in head.query_generator.state_dict()]
        without = {k: v for k, v in base.items() if not k.startswith('query_generator.')}
        missing, unexpected = head.load_state_dict(without, strict=False)
        assert set(own) <= set(missing) and not unexpected
        with pytest.raises(RuntimeError, match='Missing key'):
            head.load_state_dict(without, strict=True)
    head = _head('S')
    less = {k: v for k, v in base.items() if k != 'query_generator.fc_center.bias'}
    missing, unexpected = head.load_state_dict(less, strict=False)
    assert 'query_generator.fc_center.bias' in missing and not unexpected
    more = dict(base, **{'query_generator.center_fcs.0.weight': torch.zeros(1024, 256)})
    missing, unexpected = head.load_state_dict(more, strict=False)
    assert unexpected == ['query_generator.center_fcs.0.weight']
    # a parameter that IS there with another shape is still refused by name, strict or not
    with pytest.raises(ValueError, match=r'query_generator\.fc_center\.weight is \(3, 512\)'):
        head.load_state_dict(dict(less, **{'query_generator.fc_center.weight': torch.zeros(3, 512)}), strict=False)


def test_mismatched_state_dict_is_refused_by_parameter_name():
    base = {k: torch.from_numpy(v) for k, v in synthetic.make_head_state(seed=0).items()}
    rec = KEYS['cfg1_t_c0_f2']
    head = _head('T', rec['query_generator'])
    with pytest.raises(ValueError, match=r'query_generator\.shared_fcs\.0\.weight is \(1024, 256\).*\(512, 256\)'):
        head.load_state_dict(base)
    with pytest.raises(RuntimeError, match=r'query_generator\.shared_convs\.1\.conv\.weight'):          # a missing layer: torch's strict handling
        _head('S', dict(num_shared_convs=2)).load_state_dict(base)
    with pytest.raises(ValueError, match=r'HeadEngine: the state dict has no query_generator\.shared_convs\.1\.conv\.weight'):
        qg_shape.parse(dict(num_shared_convs=2)).check_state(base, 7, 'HeadEngine')
    # the default module against a checkpoint of another trunk
    other = {k: torch.from_numpy(v) for k, v in synthetic.with_qg_shape_state(synthetic.make_head_state(seed=0), 0, rec['query_generator']).items()}
    with pytest.raises(ValueError, match=r'query_generator\.'):
        _head('T').load_state_dict(other)
    # the shape's own check, as the engine's load_state calls it
    with pytest.raises(ValueError, match=r'HeadEngine: query_generator\.fc_center\.weight is \(3, 256\).*\(3, 512\)'):
        qg_shape.parse(rec['query_generator']).check_state({**other, 'query_generator.fc_center.weight': torch.zeros(3, 256)}, 7, 'HeadEngine')
    with pytest.raises(ValueError, match=r'holds query_generator\.center_fcs\.0'):
        qg_shape.DEFAULT.check_state({**base, 'query_generator.center_fcs.0.weight': torch.zeros(1024, 256)}, 7, 'HeadEngine')
    qg_shape.DEFAULT.check_state(base, 7, 'HeadEngine')
    with pytest.raises(ValueError, match=r'query_generator\.shared_fcs\.0\.weight is \(1024, 256\).*\(1024, 2304\)'):
        qg_shape.parse(dict(with_avg_pool=False)).check_state(base, 3, 'HeadEngine')


@pytest.mark.parametrize('s', [1, 3, 7])
def test_flatten_permutation_round_trips(s):
    g = torch.Generator().manual_seed(11 + s)
    x = torch.randn((5, 256, s, s), generator=g, dtype=torch.float64)
    W = torch.randn((16, 256 * s * s), generator=g, dtype=torch.float64)
    perm = qg_shape.flatten_perm(s)
    assert sorted(perm.tolist()) == list(range(256 * s * s))
    cells = x.flatten(2).transpose(1, 2).flatten(1)                            # the engine's cell-major rows [R, s*s*256]
    assert torch.equal(cells, x.flatten(1)[:, perm])
    # the same products summed in another order: each fp64 sum of K terms is within K * 2^-53 * sum |a_i b_i| of the exact one (the standard
    # bound of recursive summation, whatever the order or blocking of the BLAS), so two orders differ by at most twice that
    K = 256 * s * s
    bound = 2.0 * K * 2.0 ** -53 * (cells.abs() @ W[:, perm].abs().T)
    assert bool(((cells @ W[:, perm].T - x.flatten(1) @ W.T).abs() <= bound).all())


def test_goldens_load_with_documented_keys():
    rn = load_golden('qg_shape_refnoise')
    for case in CASES:
        g = load_golden('qg_shape_' + case)
        rec = KEYS[case]
        assert int(g['roi_size']) == rec['roi_size'] and synthetic.WORKLOADS[rec['problem']][0] == rec['kind']
        R = g['intr'].shape[0]
        assert g['center_pred'].shape == (R, 3) and g['xyz'].shape == (R, 3) and g['cls'].size == 6 * R * 10
        n = len(g['labels'])
        assert g['topk_index'].shape == (n,) and rn[case + '_s0_topk_index'].shape == (5, n)
        assert int(rn[case + '_s0_pairwise_ranked_diff'].max()) <= 4           # the project's NOISE_MAX
        assert os.path.getsize(os.path.join(GOLDEN, f'qg_shape_{case}.npz')) < 200 * 1024
    g = load_golden('qg_shape_micro_s_c2')
    R = g['intr'].shape[0]
    for i in (0, 1):
        assert g[f'conv{i}_pooled'].shape == (R, 256) and g[f'conv{i}_cells'].shape == (len(g[f'conv{i}_cell_rois']), 49, 256)
        assert float(g[f'conv{i}_cells'].min()) >= 0.0                        # behind the ReLU
        np.testing.assert_allclose(g[f'conv{i}_cells'].mean(1), g[f'conv{i}_pooled'][g[f'conv{i}_cell_rois']], rtol=0, atol=1e-6)
    t = load_golden('qg_shape_train')
    for name, case in (('train_micro_s', 'micro_s_c2'), ('train_cfg1_t', 'cfg1_t_c0_f2')):
        names = [str(n) for n in t[name + '.grad_names']]
        assert all('query_generator.' + k in names for k in KEYS[case]['params'])
        assert t[name + '.match'].shape[0] == 6 and any(k.startswith(name + '.loss.') for k in t)


def test_new_entries_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    lib = _lib.load()
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mv2d_hip.h')).read(), flags=re.S)
    for n in NEW_ENTRIES:
        assert re.search(r'\b' + n + r'\s*\(', hdr), n
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert lib.mv2d_abi_version() == 6
    # argument checks run before any device call
    one = (__import__('ctypes').c_double * 8)()
    assert lib.mv2d_qg_conv_cells(one, one, one, one, None, None, 1, 15, None) == -1 and b'roi_size' in lib.mv2d_last_error()
    assert lib.mv2d_qg_conv_cells(one, one, one, None, None, None, 1, 7, None) == -1              # no output at all
    assert lib.mv2d_qg_conv_cells_x3(one, one, one, one, one, None, one, None, 1, 7, None) == -1  # lo rows without hi rows
    assert lib.mv2d_avgpool_cells(one, None, one, 256, 1, 197, None) == -1 and b'cells' in lib.mv2d_last_error()
    assert lib.mv2d_avgpool_cells(one, None, one, 128, 1, 49, None) == -1
