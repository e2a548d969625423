"""Branch depth (CrossAttentionBoxHead(num_reg_fcs=1..3)) on CPU: the plugin head builds exactly the parameters of the reference module
(tests/golden/branch_depth_state_keys.json, recorded by tools/gen_golden_branch_depth.py), the shipped depth stays what it is, bad values and a
state dict of another depth are refused by name; the golden files are consistent and DECIDABLE; the synthetic helper is additive; the three C
entries check their arguments before touching memory."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import mv2d_amd
from conftest import GOLDEN, load_golden
from mv2d_amd import configs, ops, synthetic

KEYS = json.load(open(os.path.join(GOLDEN, 'branch_depth_state_keys.json')))
CASES = ['n1_cfg1_s', 'n3_cfg1_t', 'n1_rl_cfg1_t', 'n3_rl_cfg1_s']
BAD = [0, 4, -1, 2.0, True, '2']
DIMS = (2, 2, 1, 1, 2, 2)


def tol_cls(n):
    """the class-logit bound of the golden tests for the shipped two-linear chain (3e-6), in proportion to the split-precision linears of a
    deeper chain, no tighter for a shallower one"""
    return 3e-6 * max(n, 2) / 2


def _head(kind, n=2, dims=None):
    cfg = (configs.roi_head_cfg_s if kind == 'S' else configs.roi_head_cfg_t)(num_reg_fcs=n, reg_layer_dims=dims)
    return mv2d_amd.build_head(cfg, test_cfg=configs.TEST_CFG_RCNN)


def _shapes(module):
    return {k: list(v.shape) for k, v in module.state_dict().items()}


def _dims(rec):
    return tuple(rec['group_reg_dims']) if rec['group_reg_dims'] else None


@pytest.mark.parametrize('case', CASES)
def test_head_has_the_reference_parameters(case):
    rec = KEYS[case]
    n, dims = rec['num_reg_fcs'], _dims(rec)
    head = _head(rec['kind'], n, dims)
    assert head.bbox_head.num_reg_fcs == n and head.bbox_head.use_reg_layer == (dims is not None)
    assert _shapes(head.bbox_head) == rec['bbox_head']
    # the synthetic weights of that depth load strictly
    sd = synthetic.with_branch_depth_state(synthetic.make_head_state(seed=0), 0, n, dims)
    missing, unexpected = head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not missing and not unexpected
    # the key names the issue lists for layer 0
    names = {k[len('cls_branches.0.'):].split('.')[0] for k in rec['bbox_head'] if k.startswith('cls_branches.0.')}
    assert names == {str(j) for i in range(n) for j in (3 * i, 3 * i + 1)} | {str(3 * n)}
    regs = {k[len('reg_branches.0.'):].rsplit('.', 1)[0] for k in rec['bbox_head'] if k.startswith('reg_branches.0.')}
    if dims is None:
        assert regs == {str(2 * i) for i in range(n + 1)}
    else:
        assert regs == {f'reg_branch.{3 * i}' for i in range(n)} | {f'task_heads.{g}.{j}' for g in range(len(dims)) for j in (0, 2)}


@pytest.mark.parametrize('kind', ['S', 'T'])
def test_explicit_depth_2_is_todays_head_and_config(kind):
    fn = configs.roi_head_cfg_s if kind == 'S' else configs.roi_head_cfg_t
    assert fn(num_reg_fcs=2) == fn() and 'num_reg_fcs' not in fn()['bbox_head']
    assert fn(num_reg_fcs=2, reg_layer_dims=DIMS) == fn(reg_layer_dims=DIMS)
    assert fn(num_reg_fcs=3)['bbox_head']['num_reg_fcs'] == 3
    c = fn(num_reg_fcs=1, reg_layer_dims=(2, 1, 3, 2, 2))['bbox_head']
    assert c['num_reg_fcs'] == 1 and c['use_reg_layer'] is True and c['group_reg_dims'] == (2, 1, 3, 2, 2)
    head = _head(kind, 2)
    sd = synthetic.make_head_state(seed=0)
    got = _shapes(head)
    assert set(got) == set(sd) and all(got[k] == list(v.shape) for k, v in sd.items())
    assert head.bbox_head.num_reg_fcs == 2
    cfg = fn()
    cfg['bbox_head']['num_reg_fcs'] = 2                   # the key spelled out in the head's own dict
    assert _shapes(mv2d_amd.build_head(cfg, test_cfg=configs.TEST_CFG_RCNN)) == got


@pytest.mark.parametrize('bad', BAD, ids=repr)
def test_bad_num_reg_fcs(bad):
    with pytest.raises(ValueError, match='num_reg_fcs'):
        ops.check_num_reg_fcs(bad, 'test')
    for fn in (configs.roi_head_cfg_s, configs.roi_head_cfg_t):
        with pytest.raises(ValueError, match='num_reg_fcs'):
            fn(num_reg_fcs=bad)
    cfg = configs.roi_head_cfg_s()
    cfg['bbox_head']['num_reg_fcs'] = bad
    with pytest.raises(ValueError, match='num_reg_fcs'):
        mv2d_amd.build_head(cfg, test_cfg=configs.TEST_CFG_RCNN)
    with pytest.raises(ValueError, match='num_reg_fcs'):
        synthetic.with_branch_depth_state(synthetic.make_head_state(seed=0, num_layers=1), 0, bad)


def test_good_num_reg_fcs():
    assert [ops.check_num_reg_fcs(v, 't') for v in (1, 2, 3, np.int64(3))] == [1, 2, 3, 3]


@pytest.mark.parametrize('rl', [False, True], ids=['sequential', 'reg_layer'])
def test_state_dict_and_depth_must_agree(rl):
    from mv2d_amd.engine import HeadEngine
    base = synthetic.make_head_state(seed=0, num_layers=2)
    dims = DIMS if rl else None
    states = {n: synthetic.with_branch_depth_state(base, 0, n, dims) for n in (1, 2, 3)}
    for have, sd in states.items():
        assert HeadEngine.branch_depths(sd) == (have, have)
        for want in (1, 2, 3):
            if want == have:
                HeadEngine.check_branch_depth(sd, want, rl)
                continue
            with pytest.raises(ValueError, match='num_reg_fcs') as e:
                HeadEngine.check_branch_depth(sd, want, rl)
            assert f'num_reg_fcs={want}' in str(e.value) and f'have {have}' in str(e.value)
    # the shipped state is depth 2 (and make_reg_layer_state's RegLayer too)
    shipped = synthetic.with_reg_layer_state(base, 0, DIMS) if rl else base
    HeadEngine.check_branch_depth(shipped, 2, rl)
    with pytest.raises(ValueError, match='num_reg_fcs'):
        HeadEngine.check_branch_depth(shipped, 1, rl)
    # decided by shape, not by key presence alone: a depth-1 class branch with stray tensors under the depth-2 keys 4 and 6 is still refused,
    # because the tensor under key 3 is the [num_classes, 256] output layer
    fake = dict(states[1])
    for l in range(2):
        fake[f'bbox_head.cls_branches.{l}.4.weight'] = np.ones(256, np.float32)
        fake[f'bbox_head.cls_branches.{l}.6.weight'] = np.zeros((10, 256), np.float32)
    with pytest.raises(ValueError, match='num_reg_fcs'):
        HeadEngine.check_branch_depth(fake, 2, rl)
    for bad in BAD:
        with pytest.raises(ValueError, match='num_reg_fcs'):
            HeadEngine.check_branch_depth(states[2], bad, rl)


def test_synthetic_helper_is_additive():
    base, again = synthetic.make_head_state(seed=0), synthetic.make_head_state(seed=0)
    is_branch = lambda k: k.startswith(('bbox_head.cls_branches.', 'bbox_head.reg_branches.'))
    for n, dims in ((1, None), (2, None), (3, None), (1, (2, 1, 3, 2, 2)), (3, DIMS)):
        new = synthetic.with_branch_depth_state(base, 0, n, dims)
        for k in base:                                               # the input is untouched, everything but the branches is copied
            np.testing.assert_array_equal(base[k], again[k], err_msg=k)
            if not is_branch(k):
                assert new[k] is base[k], k
        assert {k for k in new if not is_branch(k)} == {k for k in base if not is_branch(k)}
        for k, v in synthetic.with_branch_depth_state(base, 0, n, dims).items():
            np.testing.assert_array_equal(v, new[k], err_msg=k)      # seeded
        if n == 2 and dims is None:
            assert list(new) == list(base)                           # the same keys in the same places ...
            assert all(new[k].shape == base[k].shape and new[k].dtype == base[k].dtype for k in base)      # ... and the input's shapes
    nc6 = synthetic.with_branch_depth_state(synthetic.make_head_state(seed=0, num_classes=6), 0, 3)
    assert nc6['bbox_head.cls_branches.5.9.weight'].shape == (6, 256)


@pytest.mark.parametrize('case', CASES)
def test_golden_files_are_consistent_and_decidable(case):
    g = load_golden('branch_depth_' + case)
    rec = KEYS[case]
    n = rec['num_reg_fcs']
    assert set(g) == {'num_reg_fcs', 'problem_seed', 'group_reg_dims', 'next_score', 'ref', 'cls', 'reg', 'boxes', 'scores', 'labels',
                      'topk_index', 'topk_scores'}
    assert int(g['num_reg_fcs']) == n and tuple(g['group_reg_dims']) == tuple(rec['group_reg_dims'] or ())
    seed = int(g['problem_seed'])
    assert seed == rec['problem_seed'] and 0 <= seed <= 9
    prob = synthetic.make_problem(rec['problem'], seed=seed, with_feat=False)
    R = sum(len(p) for p in prob['proposals'])
    lead = (6, R, 1) if rec['kind'] == 'S' else (6, 1, R)
    assert g['ref'].shape == lead[1:] + (3,) and g['cls'].shape == lead + (10,) and g['reg'].shape == lead + (10,)
    assert all(g[k].dtype == np.float32 for k in ('ref', 'cls', 'reg', 'boxes', 'scores', 'topk_scores', 'next_score'))
    assert g['topk_index'].dtype == np.int64 and g['labels'].dtype == np.int64
    k = len(g['labels'])
    assert k == 300 and g['boxes'].shape == (k, 9) and g['scores'].shape == (k,) and g['topk_index'].shape == g['topk_scores'].shape == (k,)
    assert np.isfinite(g['reg']).all() and np.isfinite(g['cls']).all()
    assert bool((np.diff(g['topk_scores']) <= 0).all()) and int(g['topk_index'].max()) < R * 10
    assert g['next_score'].shape == () and float(g['next_score']) <= float(g['topk_scores'][-1])
    rn = load_golden('branch_depth_refnoise')
    assert rn[case + '_topk_index'].shape == (len(rn[case + '_variants']), k)
    np.testing.assert_array_equal(rn[case + '_topk_index'][0], g['topk_index'])          # the first variant is the golden run
    assert rn[case + '_pairwise_ranked_diff'].shape == (len(rn[case + '_variants']),) * 2
    assert os.path.getsize(os.path.join(GOLDEN, f'branch_depth_{case}.npz')) <= os.path.getsize(os.path.join(GOLDEN, 'attn_pairs.npz'))
    # decidability: logits within eps_n move a sigmoid score by at most eps_n / 4, so two candidates can change places only if their golden
    # scores are closer than eps_n / 2.  A golden in which many ranked neighbours are that close would let the rank check pass anything.
    eps = tol_cls(n) * float(np.abs(g['cls']).max())
    s = np.sort(np.concatenate([g['topk_scores'], [g['next_score']]]).astype(np.float64))[::-1]
    near = np.abs(np.diff(s)) < eps / 2
    close = int((np.concatenate([[False], near]) | np.concatenate([near, [False]])).sum())
    print(f'[branch_depth decidable] {case}: eps_n {eps:.2e}, {close} of 300 ranked scores have a neighbour closer than eps_n / 2 (at most 8)')
    assert close <= 8


def test_c_entries_check_their_arguments_before_touching_memory():
    """n_fcs outside 1..3, a null table and L = 0 return -1 with the entry's own name in mv2d_last_error(); no GPU needed: the device pointers
    (the value 8) are never read."""
    import __graft_entry__ as g
    g.build()
    from mv2d_amd import _lib
    lib = _lib.load()
    ct, rt, wt = (ctypes.c_void_p * 7)(*[8] * 7), (ctypes.c_void_p * 5)(*[8] * 5), (ctypes.c_void_p * 8)(*[8] * 8)
    rng = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    pr = ctypes.addressof(rng)
    gd = (ctypes.c_int * 6)(*DIMS)
    eps, zero = ctypes.c_float(1e-5), ctypes.c_float(0.0)

    def heads(n=2, cls_w=ct, reg_w=rt, L=1):
        return lib.mv2d_heads_depth_x3(8, cls_w, reg_w, 8, 8, 8, 16, L, n, 10, eps, pr, zero, None, None)

    def cls_only(n=2, cls_w=ct, L=1):
        return lib.mv2d_heads_cls_depth_x3(8, cls_w, 8, 16, L, n, 10, eps, None)

    def reg_layer(n=2, w=wt, L=1):
        return lib.mv2d_reg_layer_depth_x3(8, w, 8, 8, 16, L, n, 6, gd, pr, zero, None, None)

    for fn, name in ((heads, b'mv2d_heads_depth_x3'), (cls_only, b'mv2d_heads_cls_depth_x3'), (reg_layer, b'mv2d_reg_layer_depth_x3')):
        table = 'w' if fn is reg_layer else 'cls_w'
        for kw in (dict(n=0), dict(n=4), {table: None}, dict(L=0)):
            assert fn(**kw) == -1, (name, kw)
            msg = lib.mv2d_last_error()
            assert msg.startswith(name + b':'), (name, kw, msg)
            if 'n' in kw:
                assert b'num_reg_fcs' in msg
    assert heads(reg_w=None) == -1 and lib.mv2d_last_error().startswith(b'mv2d_heads_depth_x3:')
    # a null entry INSIDE a table is caught too (the table is host memory)
    hole = (ctypes.c_void_p * 7)(*[8, 8, 8, None, 8, 8, 8])
    assert cls_only(cls_w=hole) == -1 and lib.mv2d_last_error().startswith(b'mv2d_heads_cls_depth_x3:')
    # M = 0 is a valid empty launch at every accepted depth
    for n in (1, 2, 3):
        assert lib.mv2d_heads_depth_x3(8, ct, rt, 8, 8, 8, 0, 1, n, 10, eps, pr, zero, None, None) == 0
        assert lib.mv2d_heads_cls_depth_x3(8, ct, 8, 0, 1, n, 10, eps, None) == 0
        assert lib.mv2d_reg_layer_depth_x3(8, wt, 8, 8, 0, 1, n, 6, gd, pr, zero, None, None) == 0
    assert lib.mv2d_abi_version() == 6
