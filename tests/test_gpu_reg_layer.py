"""RegLayer regression branches (CrossAttentionBoxHead(use_reg_layer=True)) on the GPU (-m gpu): the kernel mv2d_reg_layer_x3 against an fp64
restatement, the class-only launch against the fused one, the engine against goldens of the unmodified reference built with the switch
(tests/golden/reg_layer_*.npz, tools/gen_golden_reg_layer.py), the plugin head and both training routes."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from mv2d_amd import configs, synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -12345.0
PC_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)
DEFAULT = (2, 2, 1, 1, 2, 2)
# the golden bounds of tests/test_gpu_golden.py (TOL['reg'], TOL['box']) and the class-logit bound of the index-exact route
TOL_REG, TOL_BOX, TOL_CLS = 1.5e-4, 5e-3, 3e-6
# the shipped reg chain (two split-precision linears + an fp32 output layer) is held to 5e-5 relative; this one has three
TOL_KERNEL = 7.5e-5


def relerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def rnd(shape, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def _guarded(n, guard=4096):
    buf = torch.full((n + guard,), SENTINEL, device=DEV)
    return buf, buf[:n]


# ---------------------------------------------------------------------------------------------------------- the chain in torch (fp64 by dtype)
def box_code(t, ref, dt_rows=None):
    """cross_attention_head.py:216-238 + mv2d_t_head.py:136-140 on the raw code t [L,M,10], ref [M,3]"""
    x = ref.clamp(0, 1)
    inv = torch.log(x.clamp(min=1e-5) / (1 - x).clamp(min=1e-5))
    lo, hi = t.new_tensor(PC_RANGE[:3]), t.new_tensor(PC_RANGE[3:])
    cxy = torch.sigmoid(t[..., 0:2] + inv[:, 0:2]) * (hi[:2] - lo[:2]) + lo[:2]
    cz = torch.sigmoid(t[..., 4:5] + inv[:, 2:3]) * (hi[2] - lo[2]) + lo[2]
    vel = t[..., 8:] if dt_rows is None else t[..., 8:] / dt_rows[None, :, None]
    return torch.cat([cxy, t[..., 2:4], cz, t[..., 5:8], vel], -1)


def reg_layer_raw(P, outs, dims):
    """RegLayer of every layer on outs [L,M,256]: P maps 'reg_branches.{l}....' (no prefix) to tensors of outs' dtype"""
    lin = lambda x, n: x @ P[n + '.weight'].T + P[n + '.bias']
    res = []
    for l in range(outs.shape[0]):
        p = f'reg_branches.{l}.'
        feat = torch.relu(lin(torch.relu(lin(outs[l], p + 'reg_branch.0')), p + 'reg_branch.3'))
        res.append(torch.cat([lin(torch.relu(lin(feat, f'{p}task_heads.{g}.0')), f'{p}task_heads.{g}.2') for g in range(len(dims))], -1))
    return torch.stack(res)


@functools.lru_cache(maxsize=None)
def _weights(L, dims):
    """(fp32 CPU parameter dict without the 'bbox_head.' prefix, device tensors of the kernel's weight table)"""
    from mv2d_amd import ops
    sd = {k[len('bbox_head.'):]: torch.from_numpy(v) for k, v in synthetic.make_reg_layer_state(3, L, dims).items()}
    G = len(dims)
    st = lambda fmt: torch.stack([sd[fmt.format(l)] for l in range(L)]).to(DEV)
    stg = lambda fmt, join: torch.stack([join([sd[fmt.format(l, g)] for g in range(G)]) for l in range(L)]).to(DEV)
    table = ops.pack_reg_layer(st('reg_branches.{}.reg_branch.0.weight'), st('reg_branches.{}.reg_branch.0.bias'),
                               st('reg_branches.{}.reg_branch.3.weight'), st('reg_branches.{}.reg_branch.3.bias'),
                               stg('reg_branches.{}.task_heads.{}.0.weight', torch.stack), stg('reg_branches.{}.task_heads.{}.0.bias', torch.stack),
                               stg('reg_branches.{}.task_heads.{}.2.weight', torch.cat), stg('reg_branches.{}.task_heads.{}.2.bias', torch.cat))
    return sd, table


# ---------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize('dims', [DEFAULT, (2, 1, 3, 2, 2), (10,), (1,) * 10], ids=lambda d: 'g' + ''.join(map(str, d)))
@pytest.mark.parametrize('L', [1, 6])
@pytest.mark.parametrize('M', [1, 17, 77, 531, 1100])             # 531, 1100: the instances with 2 and 4 row tiles per block
def test_reg_layer_x3_vs_fp64(M, L, dims):
    from mv2d_amd import _lib, ops
    sd, table = _weights(L, dims)
    outs = rnd((L, M, 256), 51)
    ref = torch.from_numpy(np.random.Generator(np.random.PCG64(52)).random((M, 3)).astype(np.float32)) * 1.4 - 0.2
    dt_rows = torch.where(torch.arange(M) < 40, 0.5, 0.25).float()
    want = box_code(reg_layer_raw({k: v.double() for k, v in sd.items()}, outs.double(), dims), ref.double(), dt_rows.double())
    ptrs = ops.make_ptr_array(table)
    reg_buf, reg_flat = _guarded(L * M * 10)
    reg = reg_flat.view(L, M, 10)
    pcr = torch.tensor(PC_RANGE, dtype=torch.float32)
    outs_d, ref_d, dtr_d = outs.to(DEV), ref.to(DEV), dt_rows.to(DEV)
    gd = (ctypes.c_int * len(dims))(*dims)
    rc = _lib.load().mv2d_reg_layer_x3(outs_d.data_ptr(), ptrs, ref_d.data_ptr(), reg.data_ptr(), M, L, len(dims), gd, pcr.data_ptr(),
                                       ctypes.c_float(123.0), dtr_d.data_ptr(), ops._stream())
    assert rc == 0, _lib.load().mv2d_last_error()
    torch.cuda.synchronize()
    e = relerr(reg, want)
    print(f'[reg_layer_x3] M={M} L={L} dims={dims}: rel err {e:.2e} (bound {TOL_KERNEL:.1e})')
    assert bool((reg_buf[L * M * 10:] == SENTINEL).all())                            # nothing written past [L, M, 10]
    assert e < TOL_KERNEL
    # the Python wrapper reaches the same entry; without dt_rows the scalar dt divides the velocity
    reg2 = torch.empty((L, M, 10), device=DEV)
    ops.reg_layer_x3(outs_d, ptrs, ref_d, reg2, M, L, dims, pcr, dt=123.0, dt_rows=dtr_d)
    assert torch.equal(reg2, reg)
    ops.reg_layer_x3(outs_d, ptrs, ref_d, reg2, M, L, dims, pcr, dt=0.5)
    assert torch.equal(reg2[..., :8], reg[..., :8]) and torch.equal(reg2[:, :40, 8:], reg[:, :40, 8:])


def test_reg_layer_x3_rejects_bad_groups():
    from mv2d_amd import _lib, ops
    lib = _lib.load()
    _, table = _weights(1, DEFAULT)
    ptrs = ops.make_ptr_array(table)
    x = torch.zeros((1, 16, 256), device=DEV); ref = torch.zeros((16, 3), device=DEV); reg = torch.full((1, 16, 10), SENTINEL, device=DEV)
    pcr = torch.tensor(PC_RANGE, dtype=torch.float32)
    for bad in ((), (5, 6), (2, 2, 1, 1, 2), (10, 0), (3, -1, 8), (1,) * 11):
        gd = (ctypes.c_int * max(len(bad), 1))(*bad)
        rc = lib.mv2d_reg_layer_x3(x.data_ptr(), ptrs, ref.data_ptr(), reg.data_ptr(), 16, 1, len(bad), gd, pcr.data_ptr(), ctypes.c_float(0.0), None,
                                   ops._stream())
        assert rc == -1 and b'mv2d_reg_layer_x3' in lib.mv2d_last_error(), bad
        with pytest.raises(ValueError, match='group_reg_dims'):
            ops.reg_layer_x3(x, ptrs, ref, reg, 16, 1, bad, pcr)
    torch.cuda.synchronize()
    assert bool((reg == SENTINEL).all())


@pytest.mark.parametrize('M', [77, 1100])
@pytest.mark.parametrize('N', [10, 26])
def test_class_only_launch_equals_the_fused_one(N, M):
    from mv2d_amd import ops
    sdt = {k: torch.from_numpy(v) for k, v in synthetic.make_head_state(seed=0, num_classes=N).items()}
    L = 6
    outs, ref = rnd((L, M, 256), 61).to(DEV), torch.rand((M, 3), generator=torch.Generator().manual_seed(62)).to(DEV)
    st = lambda fmt: torch.stack([sdt[fmt.format(l)] for l in range(L)]).contiguous().to(DEV)
    c = {n: st('bbox_head.cls_branches.{}.' + n) for n in ('0.weight', '0.bias', '1.weight', '1.bias', '3.weight', '3.bias', '4.weight', '4.bias',
                                                         '6.weight', '6.bias')}
    r = {n: st('bbox_head.reg_branches.{}.' + n) for n in ('0.weight', '0.bias', '2.weight', '2.bias', '4.weight', '4.bias')}
    cw = [*ops.pack_x3_stack(c['0.weight']), c['0.bias'], c['1.weight'], c['1.bias'], *ops.pack_x3_stack(c['3.weight']), c['3.bias'], c['4.weight'],
          c['4.bias'], c['6.weight'], c['6.bias']]
    rw = [*ops.pack_x3_stack(r['0.weight']), r['0.bias'], *ops.pack_x3_stack(r['2.weight']), r['2.bias'], r['4.weight'], r['4.bias']]
    cp, rp = ops.make_ptr_array(cw), ops.make_ptr_array(rw)
    cls = torch.empty((L, M, N), device=DEV); reg = torch.empty((L, M, 10), device=DEV)
    pcr = torch.tensor(PC_RANGE, dtype=torch.float32)
    ops.heads_fused_x3(outs, cp, rp, ref, cls, reg, M, L, pcr, num_classes=N)
    buf, flat = _guarded(L * M * N)
    ops.heads_cls_x3(outs, cp, flat.view(L, M, N), M, L, num_classes=N)
    torch.cuda.synchronize()
    assert torch.equal(flat.view(L, M, N), cls)
    assert bool((buf[L * M * N:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------- 2. engine vs reference goldens
GOLDEN_CASES = [('cfg1_s', DEFAULT), ('cfg1_t', (2, 1, 3, 2, 2)), ('cfg3_t', DEFAULT)]
_RN = load_golden('reg_layer_refnoise')


def _state(dims, seed=0):
    return synthetic.with_reg_layer_state(synthetic.make_head_state(seed=seed), seed, dims)


def _engine(prob, dims, **kw):
    from mv2d_amd.engine import HeadEngine
    return HeadEngine(_state(dims), prob['kind'], torch.device(DEV), num_views=prob['views_per_frame'], use_reg_layer=True, group_reg_dims=dims, **kw)


def _inputs(prob):
    return torch.from_numpy(prob['feat']).to(DEV), [torch.from_numpy(np.asarray(p)) for p in prob['proposals']], prob['img_metas']


@pytest.mark.parametrize('name,dims', GOLDEN_CASES)
def test_engine_matches_reference_golden_reg_layer(name, dims):
    g = load_golden('reg_layer_' + name)
    assert tuple(g['group_reg_dims']) == dims
    key = name + '_s0'
    noise, gap = int(_RN[key + '_pairwise_ranked_diff'].max()), float(_RN[key + '_max_tie_gap'])
    prob = synthetic.make_problem(name, seed=0)
    eng = _engine(prob, dims, exact=True)
    out = eng.run(*_inputs(prob))
    torch.cuda.synchronize()
    R = out['R']
    e_cls = relerr(out['cls'][:, :R].reshape(g['cls'].shape), g['cls'])
    reg = out['reg'][:, :R].reshape(g['reg'].shape).cpu().numpy()
    if prob['frames'] > 1:
        reg = np.concatenate([reg[..., :8], reg[..., 8:] * 0.5], -1)      # golden reg: before the division by dt = 0.5 s (tests/test_gpu_golden.py)
    e_reg = relerr(reg, g['reg'])
    n = int(out['count'].item())
    labels = out['labels'][:n].cpu().numpy()
    flat = out['bbox_index'][:n].cpu().numpy() * 10 + labels
    ref = g['topk_index']
    n_idx = int((flat != ref).sum()) if len(ref) == n else -1
    eb, gb = out['boxes'][:n].double().cpu().numpy(), g['boxes']
    same_rank = flat == ref if len(ref) == n else np.zeros(n, bool)
    e_box = float(np.abs(eb - gb)[same_rank].max() / np.abs(gb).max()) if same_rank.any() else float('nan')
    print(f'[reg_layer golden] {name} {dims}: cls {e_cls:.1e} (bound {TOL_CLS:.0e}), reg {e_reg:.1e} (bound {TOL_REG:.1e}), {n_idx}/{n} ranked '
          f'(query, class) indices differ (reference against itself: {noise}), boxes {e_box:.1e} (bound {TOL_BOX:.0e})')
    assert e_cls < TOL_CLS
    assert e_reg < TOL_REG
    assert n == len(g['labels']) == len(ref)
    assert n_idx <= noise
    pos = {int(v): j for j, v in enumerate(ref)}
    for i, v in enumerate(flat):
        if int(v) != int(ref[i]):
            j = pos.get(int(v))
            assert j is not None and abs(float(g['topk_scores'][i]) - float(g['topk_scores'][j])) <= 2.5 * gap, (i, int(v))
    assert same_rank.sum() >= n - noise and e_box < TOL_BOX


def test_engine_eager_graph_batch_and_last_stage():
    prob, prob2 = synthetic.make_problem('cfg1_s', seed=0), synthetic.make_problem('cfg1_s', seed=5)
    keys = ('cls', 'reg', 'boxes', 'scores', 'labels', 'bbox_index', 'count')
    eng = _engine(prob, DEFAULT)
    feat, props, metas = _inputs(prob)
    feat2, props2, metas2 = _inputs(prob2)
    o = eng.run(feat, props, metas)
    eager = {k: o[k].clone() for k in keys}
    assert bool(torch.isfinite(eager['reg']).all()) and int(eager['count']) > 0
    # graph replay: captured on other boxes, replayed on these
    buf = feat2.clone()
    eng.run(buf, props2, metas2, use_graph=True)
    buf.copy_(feat)
    o = eng.run(buf, props, metas, use_graph=True)
    for k in keys:
        assert torch.equal(o[k], eager[k]), k
    # two samples through one sequence of launches
    for use_graph in (False, True):
        ob = eng.run_batch([feat, feat2], [props, props2], [metas, metas2], use_graph=use_graph)
        grp = ob['grp_start'].tolist()
        assert torch.equal(ob['cls'][:, grp[0]:grp[1]], eager['cls']) and torch.equal(ob['reg'][:, grp[0]:grp[1]], eager['reg']), use_graph
        n = int(eager['count'])
        assert int(ob['count'][0]) == n
        for k in ('boxes', 'scores', 'labels'):
            assert torch.equal(ob[k][0, :n], eager[k][:n]), (use_graph, k)
        single2 = eng.run(feat2, props2, metas2)
        assert torch.equal(ob['reg'][:, grp[1]:grp[2]], single2['reg'])
    # the last_stage_heads option evaluates the last layer only: the same last layer, the same detections
    last = _engine(prob, DEFAULT)
    last.last_stage_heads = True
    for use_graph in (False, True):
        o = last.run(feat, props, metas, use_graph=use_graph)
        assert torch.equal(o['cls'][-1], eager['cls'][-1]) and torch.equal(o['reg'][-1], eager['reg'][-1]), use_graph
        for k in ('boxes', 'scores', 'labels', 'count'):
            assert torch.equal(o[k], eager[k]), (use_graph, k)
    # the switch decides which graph runs: an engine of the default head on the same inputs gives other boxes
    from mv2d_amd.engine import HeadEngine
    plain = HeadEngine(synthetic.make_head_state(seed=0), 'S', torch.device(DEV), num_views=prob['views_per_frame'])
    assert not torch.equal(plain.run(feat, props, metas)['reg'], eager['reg'])
    with pytest.raises(ValueError, match='reg_branch'):
        HeadEngine(synthetic.make_head_state(seed=0), 'S', torch.device(DEV), num_views=2, use_reg_layer=True)
    with pytest.raises(ValueError, match='reg_branch'):
        HeadEngine(_state(DEFAULT), 'S', torch.device(DEV), num_views=2)


# ---------------------------------------------------------------------------------------------------------- 3. plugin head
def _build(kind, dims, use_denoise=None, train=False, num_views=2):
    import mv2d_amd
    cfg = (configs.roi_head_cfg_s if kind == 'S' else configs.roi_head_cfg_t)(reg_layer_dims=dims)
    if kind == 'T':
        cfg['num_views'] = num_views                  # views per frame of the micro / cfg1 problems
    if use_denoise is not None:
        cfg['use_denoise'] = use_denoise
    head = mv2d_amd.build_head(cfg, train_cfg=configs.TRAIN_CFG_RCNN if train else None, test_cfg=configs.TEST_CFG_RCNN)
    sd = _state(dims) if dims is not None else synthetic.make_head_state(seed=0)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=not train)
    return head.to(DEV)


def test_plugin_simple_test_equals_the_engine():
    dims = (2, 1, 3, 2, 2)
    head = _build('S', dims).eval()
    probs = [synthetic.make_problem('cfg1_s', seed=s) for s in (0, 4)]
    feats = [torch.from_numpy(p['feat']).to(DEV) for p in probs]
    metas = [[dict(m, box_type_3d=None) for m in p['img_metas']] for p in probs]
    props = [[torch.from_numpy(x) for x in p['proposals']] for p in probs]
    singles = [head.simple_test([feats[b]], props[b], metas[b])[0] for b in range(2)]
    eng = _engine(probs[0], dims, max_num=300)
    out = eng.run(feats[0], props[0], probs[0]['img_metas'])
    for a, w in zip(singles[0], eng.results(out)):
        assert torch.equal(a, w)
    assert len(singles[0][2]) > 0
    got = head.simple_test_batch([torch.cat(feats, 0)], props, metas)
    for b in range(2):
        for a, w in zip(got[b], singles[b]):
            assert torch.equal(a, w), b
    # the bbox head's own forward (the reference's signature) runs the RegLayer through the new launch: on the engine's decoder outputs it
    # returns the engine's box codes of every layer
    o = eng.run(feats[0], props[0], probs[0]['img_metas'], keep_stages=True)
    R, bh = o['R'], head.bbox_head
    outs = o['ws']['outs'][:, :R].clone(memory_format=torch.contiguous_format)
    bh.transformer.forward = lambda *a, **k: (outs.view(outs.shape[0], R, 1, 256), None)      # (S path: one query per RoI sample)
    z = torch.zeros(R, 1, 256, 1, 1, device=DEV)
    cls, reg = bh(o['ws']['ref'][:R].view(R, 1, 3).clone(), z, None, z)
    assert torch.equal(reg.reshape(-1, R, 10), o['reg'][:, :R])
    assert relerr(cls.reshape(-1, R, 10), o['cls'][:, :R]) < 5e-5                       # (fp32 class branch of forward vs the split-precision launch)


# ---------------------------------------------------------------------------------------------------------- 4. training
def _dropout_off(head):
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    return head


def _reg_layer_parameters(head):
    return {n: p for n, p in head.named_parameters() if '.reg_branches.' in n}


@pytest.mark.parametrize('name,kind,with_dn', [('micro_s', 'S', False), ('micro_t', 'T', True)])
def test_forward_train_with_reg_layer(name, kind, with_dn):
    dims = DEFAULT if kind == 'S' else (2, 1, 3, 2, 2)
    G, seed = 5, 31
    head = _dropout_off(_build(kind, dims, use_denoise=with_dn, train=True))
    prob = synthetic.make_problem(name, seed=0)
    gtc = synthetic.make_train_gt(G, seed)
    gt_list, gt_labels = [torch.from_numpy(gtc['gt'])], torch.from_numpy(gtc['gt_labels'])
    rnd_ = torch.from_numpy(synthetic.make_dn_noise(G * 10, seed)).to(DEV)
    feat = torch.from_numpy(prob['feat']).to(DEV)
    props = [torch.from_numpy(p) for p in prob['proposals']]
    metas = [dict(m, box_type_3d=None) for m in prob['img_metas']]
    args = ([feat], metas, props, None, None, None, None, gt_list, [gt_labels], None)
    # (the Hungarian assignment of the first route is reused by the second: a near-tie may flip under their rounding difference)
    hl = head._head_loss(torch.device('cuda', torch.cuda.current_device()))
    seen, orig_assign = {}, hl.assigner.assign

    def record(*a, **k):
        seen['match'] = orig_assign(*a, **k)
        return seen['match']
    hl.assigner.assign = record
    with torch.no_grad():
        fwd = head.forward_train(*args, dn_noise=rnd_, autograd=False)
    hl.assigner.assign = lambda *a, **k: seen['match']
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in fwd.values())
    assert any(k.endswith('dn_loss_bbox') for k in fwd) == with_dn
    head.zero_grad(set_to_none=True)
    losses = head.forward_train(*args, dn_noise=rnd_, autograd=True)
    assert set(losses) == set(fwd)
    for k in fwd:      # the two routes agree (16-bit K / V on the autograd route only; the bound of tests/test_gpu_train.py for the two routes)
        assert abs(float(fwd[k]) - float(losses[k])) <= 5e-3 * max(abs(float(fwd[k])), 1e-2), (k, float(fwd[k]), float(losses[k]))
    sum(losses.values()).backward()
    params = _reg_layer_parameters(head)
    from mv2d_amd.autograd_ops import branch_params
    want = {'bbox_head.' + n.format(l=l) for l in range(6) for n in branch_params(True, dims)[10:]}
    assert set(params) == want and len(want) == 6 * (4 + 4 * len(dims))
    for n, p in params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n


def _seq_raw(P, outs):
    lin = lambda x, n: x @ P[n + '.weight'].T + P[n + '.bias']
    return torch.stack([lin(torch.relu(lin(torch.relu(lin(outs[l], f'reg_branches.{l}.0')), f'reg_branches.{l}.2')), f'reg_branches.{l}.4')
                        for l in range(outs.shape[0])])


def _kind(name):
    """d_outs | w256 / b256 (the 256 x 256 linears) | w_out / b_out (the layers that write box-code columns)"""
    if name == 'd_outs':
        return name
    idx = name.split('.')[-2]
    out_layer = idx == '4' or ('task_heads' in name and idx == '2')
    return ('w' if name.endswith('weight') else 'b') + ('_out' if out_layer else '256')


def _branch_grad_errors(head, raw_fn, T=77):
    """Gradients of sum(w * box code) through TrainDecoder._branches against torch autograd on the fp64 restatement: the largest error of every
    kind of quantity (relative to the largest entry of the fp64 gradient), for the regression branches' parameters and the decoder outputs."""
    from mv2d_amd import train
    dec = train.TrainDecoder(head)
    L = dec.L
    outs = rnd((L, T, 256), 71).to(DEV).requires_grad_(True)
    ref = (torch.from_numpy(np.random.Generator(np.random.PCG64(72)).random((T, 3)).astype(np.float32)) * 0.9 + 0.05).to(DEV)
    wb = rnd((L, T, 10), 73).to(DEV)
    head.zero_grad(set_to_none=True)
    _, box = dec._branches(outs, ref, 0, 0.0)
    (box * wb).sum().backward()
    P = {n[len('bbox_head.'):]: p for n, p in head.named_parameters() if '.reg_branches.' in n}
    P64 = {n: p.detach().double().cpu().requires_grad_(True) for n, p in P.items()}
    o64 = outs.detach().double().cpu().requires_grad_(True)
    box64 = box_code(raw_fn(P64, o64), ref.double().cpu())
    e_fwd = relerr(box, box64)
    (box64 * wb.double().cpu()).sum().backward()
    errs = {'fwd': e_fwd}
    for n, g, w in [('d_outs', outs.grad, o64.grad)] + [(n, P[n].grad, P64[n].grad) for n in P]:
        assert g is not None and bool(torch.isfinite(g).all()), n
        k = _kind(n)
        errs[k] = max(errs.get(k, 0.0), relerr(g, w))
    return errs


def test_reg_layer_gradients_match_fp64_autograd():
    """tests/test_gpu_train.py holds the operators (5e-5 per linear) and the whole step (against the reference's goldens), not the branches on
    their own; so: the same heads-only function through the shipped HeadsFn node and through the RegLayer's per-operator nodes, each against
    torch autograd on its fp64 restatement, and the RegLayer route may show twice the shipped route's error for every kind of quantity."""
    dims = (2, 1, 3, 2, 2)
    shipped = _branch_grad_errors(_dropout_off(_build('S', None, train=True)), _seq_raw)
    new = _branch_grad_errors(_dropout_off(_build('S', dims, train=True)), lambda P, o: reg_layer_raw(P, o, dims))
    print('[reg_layer grads] shipped HeadsFn vs fp64: ' + ', '.join(f'{k} {v:.2e}' for k, v in sorted(shipped.items())))
    print('[reg_layer grads] RegLayer route vs fp64:  ' + ', '.join(f'{k} {v:.2e}' for k, v in sorted(new.items())))
    assert set(new) == set(shipped) == {'fwd', 'd_outs', 'w256', 'b256', 'w_out', 'b_out'}
    for k in new:
        assert new[k] <= 2.0 * shipped[k], (k, new[k], shipped[k])
