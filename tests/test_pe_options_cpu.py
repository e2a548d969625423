"""The PE's with_fpe / no_sin_enc / adapt_pos3d / LID keys on CPU: the config helpers set exactly the non-default keys, ``PE`` builds the reference's
submodules for every accepted combination, everything else is refused by name (``ops.check_pe_options`` is the one list), a state dict that
disagrees with the switches is refused in both directions, ``calib.shape_tables(lid=False)`` gives the uniform bins in fp64, the goldens of
tools/gen_golden_pe_options*.py load with their documented keys, and the gate-less C entry is declared and exported."""
import itertools
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
KEYS = ('with_fpe', 'no_sin_enc', 'adapt_pos3d', 'LID')
# the 12 accepted combinations: everything but adapt_pos3d=False with no_sin_enc=False
ACCEPTED = [dict(zip(KEYS, v)) for v in itertools.product((True, False), repeat=4) if v[2] or v[1]]
CASES = {'micro_s_nofpe': ('micro_s', dict(with_fpe=False)),
         'cfg1_t_nofpe': ('cfg1_t', dict(with_fpe=False)),
         'cfg1_s_nosin_uni': ('cfg1_s', dict(no_sin_enc=True, LID=False)),
         'micro_t_plain_d40': ('micro_t', dict(with_fpe=False, no_sin_enc=True, adapt_pos3d=False, LID=False, depth_num=40))}
PE_CFG = dict(positional_encoding=dict(type='SinePositionalEncoding3D', num_feats=128, normalize=True), strides=[16])
NON_BOOLS = (0, 1, None, 'False')


def _pe(**kw):
    from mv2d_amd.plugin.modules import PE
    return PE(**{**PE_CFG, 'position_range': configs.POST_RANGE, 'depth_num': 64, **kw})


def test_there_are_12_accepted_combinations():
    assert len(ACCEPTED) == 12


def test_config_helpers_set_exactly_the_non_default_keys():
    for fn in (configs.roi_head_cfg_s, configs.roi_head_cfg_t):
        base = fn()
        assert base['pe'] == dict(PE_CFG, strides=configs.ROI_STRIDES, position_range=configs.POST_RANGE, depth_num=64, with_fpe=True)
        assert fn(with_fpe=True, no_sin_enc=False, adapt_pos3d=True, LID=True) == base               # the defaults: today's dict
        for combo in ACCEPTED:
            cfg = fn(**combo)
            want = dict(base['pe'])
            want.update({k: v for k, v in combo.items() if v != ops.PE_OPTION_DEFAULTS[k]})
            assert cfg['pe'] == want, combo
            assert set(cfg['pe']) - set(base['pe']) == {k for k in KEYS[1:] if combo[k] != ops.PE_OPTION_DEFAULTS[k]}
            cfg['pe'] = base['pe']
            assert cfg == base                                                                         # nothing else moved
        cfg = fn(with_fpe=False, depth_num=40, depth_start=2.0, num_classes=6)                        # combines with the other keys
        assert cfg['pe']['with_fpe'] is False and cfg['pe']['depth_num'] == 40 and cfg['pe']['depth_start'] == 2.0
        assert cfg['bbox_head']['num_classes'] == 6


def test_pe_with_fpe_false_builds():
    """The reference PE's own default (MU/pe.py:52): no fpe submodule."""
    pe = _pe(with_fpe=False)
    assert not hasattr(pe, 'fpe') and pe.with_fpe is False
    assert not any(k.startswith('fpe.') for k in pe.state_dict())
    assert hasattr(pe, 'adapt_pos3d') and hasattr(pe, 'positional_encoding')
    assert _pe().with_fpe is False                                        # (the constructor's default is the reference's)


@pytest.mark.parametrize('combo', ACCEPTED, ids=lambda c: ''.join('FT'[v] for v in c.values()))
def test_pe_builds_the_reference_submodules(combo):
    pe = _pe(**combo)
    assert hasattr(pe, 'fpe') == combo['with_fpe']
    assert hasattr(pe, 'adapt_pos3d') == (not combo['no_sin_enc']) and hasattr(pe, 'positional_encoding') == (not combo['no_sin_enc'])
    assert pe.with_fpe == combo['with_fpe'] and pe.no_sin_enc == combo['no_sin_enc'] and pe.LID == combo['LID']
    names = {k.split('.')[0] for k in pe.state_dict()}
    assert names == {'position_encoder'} | ({'fpe'} if combo['with_fpe'] else set()) | (set() if combo['no_sin_enc'] else {'adapt_pos3d'})
    assert ops.check_pe_options(**combo) == tuple(combo[k] for k in KEYS)


@pytest.mark.parametrize('case', list(CASES))
def test_pe_state_dict_equals_the_reference_modules(case):
    ref = json.load(open(os.path.join(GOLDEN, 'pe_options_state_keys.json')))
    assert set(ref) == set(CASES)
    problem, keys = CASES[case]
    rec = ref[case]
    assert rec['problem'] == problem and rec['depth_num'] == keys.get('depth_num', 64)
    for k in KEYS:
        assert rec[k] == keys.get(k, ops.PE_OPTION_DEFAULTS[k])
    pe = _pe(**{'with_fpe': True, **keys})                               # (the case's keys over the shipped config's with_fpe=True)
    assert {k: list(v.shape) for k, v in pe.state_dict().items()} == rec['position_encoding']
    # the whole head: the synthetic state laid out for the switches loads strictly
    cfg_fn = configs.roi_head_cfg_t if rec['kind'] == 'T' else configs.roi_head_cfg_s
    head = mv2d_amd.build_head(cfg_fn(**keys), test_cfg=configs.TEST_CFG_RCNN)
    sd = synthetic.make_head_state(seed=0)
    if 'depth_num' in keys:
        sd = synthetic.with_pe_depth_state(sd, 0, keys['depth_num'])
    sd = synthetic.with_pe_options_state(sd, keys.get('with_fpe', True), keys.get('no_sin_enc', False))
    missing, unexpected = head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not missing and not unexpected


def test_with_pe_options_state_only_drops_keys():
    base = synthetic.make_head_state(seed=0)
    assert set(synthetic.with_pe_options_state(base)) == set(base)
    a = synthetic.with_pe_options_state(base, with_fpe=False)
    assert set(base) - set(a) == {k for k in base if k.startswith('position_encoding.fpe.')} and len(set(base) - set(a)) == 4
    b = synthetic.with_pe_options_state(base, no_sin_enc=True)
    assert set(base) - set(b) == {k for k in base if k.startswith('position_encoding.adapt_pos3d.')} and len(set(base) - set(b)) == 4
    c = synthetic.with_pe_options_state(base, False, True)
    assert set(c) == set(a) & set(b) and all(c[k] is base[k] for k in c)


# ---------------------------------------------------------------------------------------------------------- refusals
def _refusers():
    from mv2d_amd.engine import HeadEngine
    return [('PE', lambda **kw: _pe(**kw)),
            ('configs', lambda **kw: configs.roi_head_cfg_s(**kw)),
            ('configs', lambda **kw: configs.roi_head_cfg_t(**kw)),
            ('PE', lambda **kw: ops.check_pe_options(**kw)),
            ('HeadEngine', lambda **kw: ops.check_pe_options(who='HeadEngine', **kw)),
            ('HeadEngine', lambda **kw: HeadEngine({}, 'T', 'cpu', **kw))]          # (HeadEngine checks its arguments before it touches the device or the weights)


def test_adapt_pos3d_false_needs_no_sin_enc():
    for who, fn in _refusers():
        with pytest.raises(ValueError, match=who + ': adapt_pos3d=False needs no_sin_enc=True'):
            fn(adapt_pos3d=False)
        with pytest.raises(ValueError, match='adapt_pos3d'):
            fn(adapt_pos3d=False, no_sin_enc=False, with_fpe=False, LID=False)
    ops.check_pe_options(adapt_pos3d=False, no_sin_enc=True)
    _pe(adapt_pos3d=False, no_sin_enc=True)


@pytest.mark.parametrize('key', KEYS)
@pytest.mark.parametrize('bad', NON_BOOLS, ids=repr)
def test_non_bool_values_are_refused_by_name(key, bad):
    for who, fn in _refusers():
        with pytest.raises(ValueError, match=f'{who}: {key} must be True or False'):
            fn(**{key: bad})
    with pytest.raises(ValueError, match=key):
        mv2d_amd.build_head({**configs.roi_head_cfg_t(), 'pe': {**configs.roi_head_cfg_t()['pe'], key: bad}}, test_cfg=configs.TEST_CFG_RCNN)


def test_state_dict_layout_against_the_switches():
    """HeadEngine.check_pe_layout (what load_state calls first, CPU-callable like check_branch_depth): fpe.* / adapt_pos3d.* present or absent
    against with_fpe / no_sin_enc, both directions, naming the switch."""
    from mv2d_amd.engine import HeadEngine
    full = synthetic.make_head_state(seed=0)
    no_fpe = synthetic.with_pe_options_state(full, with_fpe=False)
    no_sin = synthetic.with_pe_options_state(full, no_sin_enc=True)
    plain = synthetic.with_pe_options_state(full, False, True)
    HeadEngine.check_pe_layout(full)
    HeadEngine.check_pe_layout(full, True, False)
    HeadEngine.check_pe_layout(no_fpe, False, False)
    HeadEngine.check_pe_layout(no_sin, True, True)
    HeadEngine.check_pe_layout(plain, False, True)
    for sd, fpe, nosin, pat in ((full, False, False, r'fpe\.\*.*with_fpe=False'), (no_fpe, True, False, r'no position_encoding\.fpe\.\*.*with_fpe=True'),
                                (full, True, True, r'adapt_pos3d\.\*.*no_sin_enc=True'), (no_sin, True, False, r'no position_encoding\.adapt_pos3d\.\*.*no_sin_enc=False'),
                                (plain, True, True, 'with_fpe=True'), (plain, False, False, 'no_sin_enc=False')):
        with pytest.raises(ValueError, match=pat):
            HeadEngine.check_pe_layout(sd, fpe, nosin)


def test_route_refuses_the_64_bin_shipped_only_kernels():
    """route.resolve needs neither the library nor a GPU: the key16 mode's PE kernel and pe_rows_in_waves are built for the shipped PE only."""
    from types import SimpleNamespace
    from mv2d_amd import route
    for key, val in (('with_fpe', False), ('no_sin_enc', True), ('LID', False)):
        o = SimpleNamespace(**route.default_options())
        assert route.resolve(o, 'T', True, 64, pe_options={key: val}).pe_x3
        with pytest.raises(ValueError, match=rf'pe_tab96.*{key}='):
            route.resolve(o, 'T', False, 64, pe_options={key: val})
        o.pe_rows_in_waves = True
        with pytest.raises(ValueError, match=rf'pe_rows_in_waves.*{key}='):
            route.resolve(o, 'T', True, 64, pe_options={key: val})
    plain = SimpleNamespace(**route.default_options())
    for exact in (True, False):
        assert route.resolve(plain, 'S', exact, 64, pe_options=dict(with_fpe=True, no_sin_enc=False, LID=True)) == route.resolve(plain, 'S', exact, 64)


# ---------------------------------------------------------------------------------------------------------- uniform bins
@pytest.mark.parametrize('D,start,rng', [(64, 1, configs.POST_RANGE), (40, 2.0, [-65.0, -65.0, -8.0, 65.0, 65.0, 8.0]), (8, 0.5, configs.POST_RANGE)])
def test_shape_tables_uniform_bins(D, start, rng):
    prob = synthetic.make_problem('micro_t', seed=0)
    shapes = calib.meta_shapes(prob['img_metas'])
    _, _, h, w = prob['feat'].shape
    uni = calib.shape_tables(shapes, h, w, depth_num=D, depth_start=start, position_range=tuple(rng), lid=False)
    bin_size = (rng[3] - start) / D
    want = start + bin_size * torch.arange(0, D, 1).double()                     # MU/pe.py:101-104, fp64
    assert uni['coords_d'].dtype == torch.float64 and torch.equal(uni['coords_d'], want)
    assert float(uni['coords_d'][0]) == start
    assert abs(float(uni['coords_d'][-1]) - (rng[3] - bin_size)) <= 1e-12 * rng[3]       # the last bin is position_range[3] - bin_size
    dflt = calib.shape_tables(shapes, h, w, depth_num=D, depth_start=start, position_range=tuple(rng))
    lid = calib.shape_tables(shapes, h, w, depth_num=D, depth_start=start, position_range=tuple(rng), lid=True)
    idx = torch.arange(D).double()
    assert torch.equal(dflt['coords_d'], start + (rng[3] - start) / (D * (1 + D)) * idx * (idx + 1))
    for k in dflt:                                                                 # lid=True is today's default call; nothing else depends on the spacing
        same = (lambda a, b: torch.equal(a, b)) if torch.is_tensor(dflt[k]) else (lambda a, b: a == b)
        assert same(dflt[k], lid[k]), k
        if k != 'coords_d':
            assert same(dflt[k], uni[k]), k
    assert not torch.equal(uni['coords_d'], dflt['coords_d'])
    ft = calib.frame_tables(prob['img_metas'], h, w, depth_num=D, depth_start=start, position_range=tuple(rng), lid=False)
    assert torch.equal(ft['coords_d'], uni['coords_d'])
    assert torch.equal(calib.frame_tables(prob['img_metas'], h, w, depth_num=D, depth_start=start, position_range=tuple(rng))['coords_d'], dflt['coords_d'])


# ---------------------------------------------------------------------------------------------------------- goldens
def test_goldens_load_with_documented_keys():
    rn = load_golden('pe_options_refnoise')
    ref = json.load(open(os.path.join(GOLDEN, 'pe_options_state_keys.json')))
    assert {k.rsplit('_s', 1)[0] for k in rn if k.endswith('_variants')} == set(CASES)
    for case, (problem, keys) in CASES.items():
        g = load_golden('pe_options_' + case)
        kind = synthetic.WORKLOADS[problem][0]
        seed = int(g['seed'])
        assert seed == ref[case]['seed'] and int(g['depth_num']) == keys.get('depth_num', 64)
        for k in KEYS:
            assert bool(g[k]) == keys.get(k, ops.PE_OPTION_DEFAULTS[k])
        R = g['intr'].shape[0]
        assert g['intr'].shape == (R, 16) and g['cls'].shape[0] == 6 and g['cls'].size == 6 * R * 10 and g['reg'].shape == g['cls'].shape
        assert g['center_pred'].shape == (R, 3) and g['xyz'].shape == (R, 3)
        n = len(g['labels'])
        assert g['boxes'].shape == (n, 9) and g['scores'].shape == (n,) and g['topk_index'].shape == (n,) and g['topk_scores'].shape == (n,)
        assert ('feat_for_rois' in g and 'key_padding' in g) if kind == 'T' else ('corr' in g and 'corr_mask' in g)
        key = f'{case}_s{seed}'
        assert int(rn[key + '_pairwise_ranked_diff'].max()) <= 4           # the project's NOISE_MAX: a condition of the generator
        assert rn[key + '_topk_index'].shape == (5, n) and float(rn[key + '_max_tie_gap']) >= 0.0
        assert os.path.getsize(os.path.join(GOLDEN, f'pe_options_{case}.npz')) < 200 * 1024
        if problem.startswith('micro'):
            assert g['pe_rows'].shape == (len(g['pe_positions']), 256) and int(g['pe_positions'].max()) < 2 * 8 * 12
            assert np.array_equal(g['pe_positions'], np.arange(0, 2 * 8 * 12, 3))
        else:
            assert 'pe_rows' not in g
    for f in ('pe_options_refnoise.npz', 'pe_options_train.npz', 'pe_options_state_keys.json'):
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 200 * 1024
    t = load_golden('pe_options_train')
    for name, gone in (('train_micro_t', '.fpe.'), ('train_micro_s', '.adapt_pos3d.')):
        names = [str(n) for n in t[name + '.grad_names']]
        assert len(names) == 228 and 'position_encoding.position_encoder.0.weight' in names and not any(gone in n for n in names)
        assert t[name + '.grad_norm'].shape == (228,) and t[name + '.grad_proj'].shape == (228,)
        assert t[name + '.match'].shape[0] == 6 and t[name + '.cls'].shape[0] == 6
        assert any(k.startswith(name + '.loss.') for k in t)
    assert any(k.startswith('train_micro_t.loss.') and 'dn_loss' in k for k in t)
    assert {k.split('.')[1] for k in t if k.startswith('train_micro_t.')} == {k.split('.')[1] for k in load_golden('pe_depth_train_d32') if k.startswith('train_micro_t.')}


# ---------------------------------------------------------------------------------------------------------- the C entry
def test_gate_less_entry_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    lib = _lib.load()
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mv2d_hip.h')).read(), flags=re.S)
    n = 'mv2d_pe_fused_x3_ng'
    assert re.search(r'\b' + n + r'\s*\(', hdr)
    assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert len(_lib.SIGNATURES[n][1]) == 24
    assert lib.mv2d_abi_version() == 6
    # argument checks run before any device call: a Kp the kernel has no instance for is an error
    for Kp in (0, 48, 288):
        assert lib.mv2d_pe_fused_x3_ng(*([None] * 4), 4, *([None] * 7), 1, *([None] * 5), 0, 0, None, 0, Kp, None) == -1
        assert b'Kp' in lib.mv2d_last_error()
