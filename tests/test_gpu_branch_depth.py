"""Branch depth (CrossAttentionBoxHead(num_reg_fcs=1..3)) on the GPU (-m gpu): the depth entries of csrc/branches_x3.hip against fp64
restatements and, at depth 2, bit for bit against the shipped launches; the engine against goldens of the unmodified reference built with the key
(tests/golden/branch_depth_*.npz, tools/gen_golden_branch_depth.py); engine consistency, the plugin head and both training routes.

Bounds (tests/test_gpu_reg_layer.py:21-22: a chain's bound against fp64 grows with its number of split-precision linears, and a shallower chain
gets no tighter bound than the shipped one): 5e-5 for two linears, 7.5e-5 for three, 1e-4 for four; TOL_CLS 3e-6 and TOL_REG 1.5e-4 of the golden
tests times max(n, 2) / 2; TOL_BOX 5e-3."""
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
TOL_BOX = 5e-3


def tol_chain(linears):
    """2.5e-5 per split-precision linear of the chain, at least the shipped two-linear chain's 5e-5"""
    return 2.5e-5 * max(linears, 2)


def tol_cls(n):
    return 3e-6 * max(n, 2) / 2


def tol_reg(n):
    return 1.5e-4 * max(n, 2) / 2


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


def _pcr():
    return torch.tensor(PC_RANGE, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------- the chains in torch (fp64 by dtype)
def box_code(t, ref, dt_rows=None):
    """cross_attention_head.py:216-238 + mv2d_t_head.py:136-140 on the raw code t [L,M,10], ref [M,3]"""
    x = ref.clamp(0, 1)
    inv = torch.log(x.clamp(min=1e-5) / (1 - x).clamp(min=1e-5))
    lo, hi = t.new_tensor(PC_RANGE[:3]), t.new_tensor(PC_RANGE[3:])
    cxy = torch.sigmoid(t[..., 0:2] + inv[:, 0:2]) * (hi[:2] - lo[:2]) + lo[:2]
    cz = torch.sigmoid(t[..., 4:5] + inv[:, 2:3]) * (hi[2] - lo[2]) + lo[2]
    vel = t[..., 8:] if dt_rows is None else t[..., 8:] / dt_rows[None, :, None]
    return torch.cat([cxy, t[..., 2:4], cz, t[..., 5:8], vel], -1)


def _lin(P, x, name):
    return x @ P[name + '.weight'].T + P[name + '.bias']


def cls_raw(P, outs, n):
    res = []
    for l in range(outs.shape[0]):
        p, y = f'cls_branches.{l}.', outs[l]
        for i in range(n):
            y = torch.relu(torch.nn.functional.layer_norm(_lin(P, y, f'{p}{3 * i}'), (256,), P[f'{p}{3 * i + 1}.weight'], P[f'{p}{3 * i + 1}.bias'], 1e-5))
        res.append(_lin(P, y, f'{p}{3 * n}'))
    return torch.stack(res)


def seq_raw(P, outs, n):
    res = []
    for l in range(outs.shape[0]):
        p, y = f'reg_branches.{l}.', outs[l]
        for i in range(n):
            y = torch.relu(_lin(P, y, f'{p}{2 * i}'))
        res.append(_lin(P, y, f'{p}{2 * n}'))
    return torch.stack(res)


def reg_layer_raw(P, outs, n, dims):
    res = []
    for l in range(outs.shape[0]):
        p, y = f'reg_branches.{l}.', outs[l]
        for i in range(n):
            y = torch.relu(_lin(P, y, f'{p}reg_branch.{3 * i}'))
        res.append(torch.cat([_lin(P, torch.relu(_lin(P, y, f'{p}task_heads.{g}.0')), f'{p}task_heads.{g}.2') for g in range(len(dims))], -1))
    return torch.stack(res)


def _state(n, dims=None, num_classes=10, L=6, seed=0):
    return synthetic.with_branch_depth_state(synthetic.make_head_state(seed=seed, num_layers=L, num_classes=num_classes), seed, n, dims)


@functools.lru_cache(maxsize=None)
def _tables(L, n, NC, dims=None):
    """(fp32 CPU parameters without the 'bbox_head.' prefix, class table, regression table) on the device, stacked [L][n] by the ops packers"""
    from mv2d_amd import ops
    sd = {k[len('bbox_head.'):]: torch.from_numpy(v) for k, v in _state(n, dims, NC, L).items() if '_branches.' in k}
    st = lambda fmt: torch.stack([sd[fmt.format(l)] for l in range(L)]).to(DEV)
    stn = lambda fmt, idx: torch.stack([torch.stack([sd[fmt.format(l, i)] for i in idx]) for l in range(L)]).to(DEV)
    lin, ln = [3 * i for i in range(n)], [3 * i + 1 for i in range(n)]
    c = 'cls_branches.{}.{}.'
    cls_args = (stn(c + 'weight', lin), stn(c + 'bias', lin), stn(c + 'weight', ln), stn(c + 'bias', ln),
                st('cls_branches.{}.' + str(3 * n) + '.weight'), st('cls_branches.{}.' + str(3 * n) + '.bias'))
    if dims is None:
        ev = [2 * i for i in range(n)]
        cls_t, reg_t = ops.pack_heads_depth(*cls_args, stn('reg_branches.{}.{}.weight', ev), stn('reg_branches.{}.{}.bias', ev),
                                            st('reg_branches.{}.' + str(2 * n) + '.weight'), st('reg_branches.{}.' + str(2 * n) + '.bias'))
        return sd, cls_t, reg_t
    G = len(dims)
    stg = lambda fmt, join: torch.stack([join([sd[fmt.format(l, g)] for g in range(G)]) for l in range(L)]).to(DEV)
    cls_t, _ = ops.pack_heads_depth(*cls_args)
    reg_t = ops.pack_reg_layer_depth(stn('reg_branches.{}.reg_branch.{}.weight', lin), stn('reg_branches.{}.reg_branch.{}.bias', lin),
                                     stg('reg_branches.{}.task_heads.{}.0.weight', torch.stack), stg('reg_branches.{}.task_heads.{}.0.bias', torch.stack),
                                     stg('reg_branches.{}.task_heads.{}.2.weight', torch.cat), stg('reg_branches.{}.task_heads.{}.2.bias', torch.cat))
    return sd, cls_t, reg_t


def _rows(M, L):
    outs = rnd((L, M, 256), 51)
    ref = torch.from_numpy(np.random.Generator(np.random.PCG64(52)).random((M, 3)).astype(np.float32)) * 1.4 - 0.2
    dt_rows = torch.where(torch.arange(M) < 40, 0.5, 0.25).float()
    return outs, ref, dt_rows


# ---------------------------------------------------------------------------------------------------------- 1. the class / Sequential chain
@pytest.mark.parametrize('NC', [1, 10, 26, 64])              # one masked tile, the shipped count, two tiles, four full tiles
@pytest.mark.parametrize('M', [1, 17, 531, 1100])            # a partial tile, a tile + 1 row, the RT = 2 and RT = 4 instances with a ragged last block
@pytest.mark.parametrize('L', [1, 6])
@pytest.mark.parametrize('n', [1, 3])
def test_heads_depth_x3_vs_fp64(n, L, M, NC):
    from mv2d_amd import _lib, ops
    sd, cls_t, reg_t = _tables(L, n, NC)
    outs, ref, dt_rows = _rows(M, L)
    P64 = {k: v.double() for k, v in sd.items()}
    want_cls = cls_raw(P64, outs.double(), n)
    want_reg = box_code(seq_raw(P64, outs.double(), n), ref.double(), dt_rows.double())
    cp, rp = ops.make_ptr_array(cls_t), ops.make_ptr_array(reg_t)
    cls_buf, cls_flat = _guarded(L * M * NC)
    reg_buf, reg_flat = _guarded(L * M * 10)
    cls, reg = cls_flat.view(L, M, NC), reg_flat.view(L, M, 10)
    pcr = _pcr()
    outs_d, ref_d, dtr_d = outs.to(DEV), ref.to(DEV), dt_rows.to(DEV)
    rc = _lib.load().mv2d_heads_depth_x3(outs_d.data_ptr(), cp, rp, ref_d.data_ptr(), cls.data_ptr(), reg.data_ptr(), M, L, n, NC,
                                         ctypes.c_float(1e-5), pcr.data_ptr(), ctypes.c_float(123.0), dtr_d.data_ptr(), ops._stream())
    assert rc == 0, _lib.load().mv2d_last_error()
    torch.cuda.synchronize()
    e_cls, e_reg, bound = relerr(cls, want_cls), relerr(reg, want_reg), tol_chain(n)
    print(f'[heads_depth_x3] n={n} L={L} M={M} NC={NC}: cls rel err {e_cls:.2e}, reg rel err {e_reg:.2e} (bound {bound:.1e})')
    assert bool((cls_buf[L * M * NC:] == SENTINEL).all()) and bool((reg_buf[L * M * 10:] == SENTINEL).all())      # nothing past [L,M,NC] / [L,M,10]
    assert e_cls < bound and e_reg < bound
    # the Python wrapper reaches the same entry; without dt_rows the scalar dt divides the velocity
    cls2, reg2 = torch.empty((L, M, NC), device=DEV), torch.empty((L, M, 10), device=DEV)
    ops.heads_depth_x3(outs_d, cp, rp, ref_d, cls2, reg2, M, L, n, pcr, dt=123.0, dt_rows=dtr_d, num_classes=NC)
    assert torch.equal(cls2, cls) and torch.equal(reg2, reg)
    ops.heads_depth_x3(outs_d, cp, rp, ref_d, cls2, reg2, M, L, n, pcr, dt=0.5, num_classes=NC)
    assert torch.equal(cls2, cls) and torch.equal(reg2[..., :8], reg[..., :8]) and torch.equal(reg2[:, :40, 8:], reg[:, :40, 8:])
    assert relerr(reg2, box_code(seq_raw(P64, outs.double(), n), ref.double(), torch.full((M,), 0.5).double())) < bound
    # the class-only entry: bit for bit the cls of the two-branch entry, nothing past it
    buf3, flat3 = _guarded(L * M * NC)
    ops.heads_cls_depth_x3(outs_d, cp, flat3.view(L, M, NC), M, L, n, num_classes=NC)
    torch.cuda.synchronize()
    assert torch.equal(flat3.view(L, M, NC), cls) and bool((buf3[L * M * NC:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------- 2. the RegLayer chain
@pytest.mark.parametrize('dims', [DEFAULT, (10,), (1,) * 10], ids=lambda d: 'g' + ''.join(map(str, d)))
@pytest.mark.parametrize('M', [1, 17, 531, 1100])
@pytest.mark.parametrize('L', [1, 6])
@pytest.mark.parametrize('n', [1, 3])
def test_reg_layer_depth_x3_vs_fp64(n, L, M, dims):
    from mv2d_amd import _lib, ops
    sd, _, reg_t = _tables(L, n, 10, dims)
    outs, ref, dt_rows = _rows(M, L)
    want = box_code(reg_layer_raw({k: v.double() for k, v in sd.items()}, outs.double(), n, dims), ref.double(), dt_rows.double())
    ptrs = ops.make_ptr_array(reg_t)
    reg_buf, reg_flat = _guarded(L * M * 10)
    reg = reg_flat.view(L, M, 10)
    pcr = _pcr()
    outs_d, ref_d, dtr_d = outs.to(DEV), ref.to(DEV), dt_rows.to(DEV)
    gd = (ctypes.c_int * len(dims))(*dims)
    rc = _lib.load().mv2d_reg_layer_depth_x3(outs_d.data_ptr(), ptrs, ref_d.data_ptr(), reg.data_ptr(), M, L, n, len(dims), gd, pcr.data_ptr(),
                                             ctypes.c_float(123.0), dtr_d.data_ptr(), ops._stream())
    assert rc == 0, _lib.load().mv2d_last_error()
    torch.cuda.synchronize()
    e, bound = relerr(reg, want), tol_chain(n + 1)
    print(f'[reg_layer_depth_x3] n={n} L={L} M={M} dims={dims}: rel err {e:.2e} (bound {bound:.1e})')
    assert bool((reg_buf[L * M * 10:] == SENTINEL).all())
    assert e < bound
    reg2 = torch.empty((L, M, 10), device=DEV)
    ops.reg_layer_depth_x3(outs_d, ptrs, ref_d, reg2, M, L, n, dims, pcr, dt=123.0, dt_rows=dtr_d)
    assert torch.equal(reg2, reg)
    ops.reg_layer_depth_x3(outs_d, ptrs, ref_d, reg2, M, L, n, dims, pcr, dt=0.5)
    assert torch.equal(reg2[..., :8], reg[..., :8]) and torch.equal(reg2[:, :40, 8:], reg[:, :40, 8:])


def test_wrappers_refuse_other_depths():
    from mv2d_amd import ops
    _, cls_t, reg_t = _tables(1, 1, 10)
    cp, rp = ops.make_ptr_array(cls_t), ops.make_ptr_array(reg_t)
    x = torch.zeros((1, 16, 256), device=DEV); ref = torch.zeros((16, 3), device=DEV)
    cls, reg = torch.full((1, 16, 10), SENTINEL, device=DEV), torch.full((1, 16, 10), SENTINEL, device=DEV)
    for bad in (0, 4, -1, 2.0, True, '2'):
        with pytest.raises(ValueError, match='num_reg_fcs'):
            ops.heads_depth_x3(x, cp, rp, ref, cls, reg, 16, 1, bad, _pcr())
        with pytest.raises(ValueError, match='num_reg_fcs'):
            ops.heads_cls_depth_x3(x, cp, cls, 16, 1, bad)
        with pytest.raises(ValueError, match='num_reg_fcs'):
            ops.reg_layer_depth_x3(x, rp, ref, reg, 16, 1, bad, DEFAULT, _pcr())
    torch.cuda.synchronize()
    assert bool((cls == SENTINEL).all()) and bool((reg == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------- 3. depth 2 = the shipped launches
@pytest.mark.parametrize('M', [77, 1100])
@pytest.mark.parametrize('NC', [10, 26])
def test_depth_2_equals_the_shipped_launches(NC, M):
    """An indexing or ordering slip in the depth loop shows here bit for bit where a tolerance would hide it."""
    from mv2d_amd import ops
    L, n = 6, 2
    pcr = _pcr()
    outs, ref, dt_rows = (t.to(DEV) for t in _rows(M, L))
    # Sequential: the head state make_head_state draws, in the shipped tables and in the [L][n] ones
    sdt = {k: torch.from_numpy(v) for k, v in synthetic.make_head_state(seed=0, num_classes=NC).items()}
    st = lambda fmt: torch.stack([sdt[fmt.format(l)] for l in range(L)]).contiguous().to(DEV)
    c = {k: st('bbox_head.cls_branches.{}.' + k) for k in ('0.weight', '0.bias', '1.weight', '1.bias', '3.weight', '3.bias', '4.weight', '4.bias',
                                                         '6.weight', '6.bias')}
    r = {k: st('bbox_head.reg_branches.{}.' + k) for k in ('0.weight', '0.bias', '2.weight', '2.bias', '4.weight', '4.bias')}
    cw = [*ops.pack_x3_stack(c['0.weight']), c['0.bias'], c['1.weight'], c['1.bias'], *ops.pack_x3_stack(c['3.weight']), c['3.bias'], c['4.weight'],
          c['4.bias'], c['6.weight'], c['6.bias']]
    rw = [*ops.pack_x3_stack(r['0.weight']), r['0.bias'], *ops.pack_x3_stack(r['2.weight']), r['2.bias'], r['4.weight'], r['4.bias']]
    two = lambda a, b: torch.stack([a, b], 1)
    cls_t, reg_t = ops.pack_heads_depth(two(c['0.weight'], c['3.weight']), two(c['0.bias'], c['3.bias']), two(c['1.weight'], c['4.weight']),
                                        two(c['1.bias'], c['4.bias']), c['6.weight'], c['6.bias'],
                                        two(r['0.weight'], r['2.weight']), two(r['0.bias'], r['2.bias']), r['4.weight'], r['4.bias'])
    cls0, reg0 = torch.empty((L, M, NC), device=DEV), torch.empty((L, M, 10), device=DEV)
    ops.heads_fused_x3(outs, ops.make_ptr_array(cw), ops.make_ptr_array(rw), ref, cls0, reg0, M, L, pcr, dt=0.0, dt_rows=dt_rows, num_classes=NC)
    cb, cf = _guarded(L * M * NC)
    rb, rf = _guarded(L * M * 10)
    cp = ops.make_ptr_array(cls_t)
    ops.heads_depth_x3(outs, cp, ops.make_ptr_array(reg_t), ref, cf.view(L, M, NC), rf.view(L, M, 10), M, L, n, pcr, dt=0.0, dt_rows=dt_rows, num_classes=NC)
    torch.cuda.synchronize()
    assert torch.equal(cf.view(L, M, NC), cls0) and torch.equal(rf.view(L, M, 10), reg0)
    assert bool((cb[L * M * NC:] == SENTINEL).all()) and bool((rb[L * M * 10:] == SENTINEL).all())
    cls1, cls2 = torch.empty_like(cls0), torch.empty_like(cls0)
    ops.heads_cls_x3(outs, ops.make_ptr_array(cw), cls1, M, L, num_classes=NC)
    ops.heads_cls_depth_x3(outs, cp, cls2, M, L, n, num_classes=NC)
    assert torch.equal(cls2, cls1) and torch.equal(cls2, cls0)
    # RegLayer: make_reg_layer_state's branches in the shipped table and in the [L][n] one
    for dims in (DEFAULT, (2, 1, 3, 2, 2)):
        rl = {k: torch.from_numpy(v) for k, v in synthetic.make_reg_layer_state(3, L, dims).items()}
        G = len(dims)
        s1 = lambda fmt: torch.stack([rl['bbox_head.reg_branches.' + fmt.format(l)] for l in range(L)]).to(DEV)
        sg = lambda fmt, join: torch.stack([join([rl['bbox_head.reg_branches.' + fmt.format(l, g)] for g in range(G)]) for l in range(L)]).to(DEV)
        heads = (sg('{}.task_heads.{}.0.weight', torch.stack), sg('{}.task_heads.{}.0.bias', torch.stack),
                 sg('{}.task_heads.{}.2.weight', torch.cat), sg('{}.task_heads.{}.2.bias', torch.cat))
        t0 = ops.pack_reg_layer(s1('{}.reg_branch.0.weight'), s1('{}.reg_branch.0.bias'), s1('{}.reg_branch.3.weight'), s1('{}.reg_branch.3.bias'), *heads)
        t1 = ops.pack_reg_layer_depth(two(s1('{}.reg_branch.0.weight'), s1('{}.reg_branch.3.weight')),
                                      two(s1('{}.reg_branch.0.bias'), s1('{}.reg_branch.3.bias')), *heads)
        want, got = torch.empty((L, M, 10), device=DEV), torch.empty((L, M, 10), device=DEV)
        ops.reg_layer_x3(outs, ops.make_ptr_array(t0), ref, want, M, L, dims, pcr, 0.0, dt_rows=dt_rows)
        ops.reg_layer_depth_x3(outs, ops.make_ptr_array(t1), ref, got, M, L, n, dims, pcr, 0.0, dt_rows=dt_rows)
        assert torch.equal(got, want), dims


# ---------------------------------------------------------------------------------------------------------- 4. engine vs reference goldens
# (case, problem, num_reg_fcs, group_reg_dims or None): tools/gen_golden_branch_depth.py
GOLDEN_CASES = [('n1_cfg1_s', 'cfg1_s', 1, None), ('n3_cfg1_t', 'cfg1_t', 3, None),
                ('n1_rl_cfg1_t', 'cfg1_t', 1, (2, 1, 3, 2, 2)), ('n3_rl_cfg1_s', 'cfg1_s', 3, DEFAULT)]
_RN = load_golden('branch_depth_refnoise')


def _engine(prob, n, dims, **kw):
    from mv2d_amd.engine import HeadEngine
    rl = dict(use_reg_layer=True, group_reg_dims=dims) if dims else {}
    return HeadEngine(_state(n, dims), prob['kind'], torch.device(DEV), num_views=prob['views_per_frame'], num_reg_fcs=n, **rl, **kw)


def _inputs(prob):
    return torch.from_numpy(prob['feat']).to(DEV), [torch.from_numpy(np.asarray(p)) for p in prob['proposals']], prob['img_metas']


@pytest.mark.parametrize('case,problem,n,dims', GOLDEN_CASES, ids=[c[0] for c in GOLDEN_CASES])
def test_engine_matches_reference_golden(case, problem, n, dims):
    g = load_golden('branch_depth_' + case)
    assert int(g['num_reg_fcs']) == n and tuple(g['group_reg_dims']) == tuple(dims or ())
    noise, gap = int(_RN[case + '_pairwise_ranked_diff'].max()), float(_RN[case + '_max_tie_gap'])
    prob = synthetic.make_problem(problem, seed=int(g['problem_seed']))
    eng = _engine(prob, n, dims, exact=True)
    out = eng.run(*_inputs(prob))
    torch.cuda.synchronize()
    R = out['R']
    e_cls = relerr(out['cls'][:, :R].reshape(g['cls'].shape), g['cls'])
    reg = out['reg'][:, :R].reshape(g['reg'].shape).cpu().numpy()
    if prob['frames'] > 1:
        reg = np.concatenate([reg[..., :8], reg[..., 8:] * 0.5], -1)      # golden reg: before the division by dt = 0.5 s (tests/test_gpu_golden.py)
    e_reg = relerr(reg, g['reg'])
    k = int(out['count'].item())
    labels = out['labels'][:k].cpu().numpy()
    flat = out['bbox_index'][:k].cpu().numpy() * 10 + labels
    ref = g['topk_index']
    n_idx = int((flat != ref).sum()) if len(ref) == k else -1
    eb, gb = out['boxes'][:k].double().cpu().numpy(), g['boxes']
    same_rank = flat == ref if len(ref) == k else np.zeros(k, bool)
    e_box = float(np.abs(eb - gb)[same_rank].max() / np.abs(gb).max()) if same_rank.any() else float('nan')
    eps = tol_cls(n) * float(np.abs(g['cls']).max())
    print(f'[branch_depth golden] {case}: cls {e_cls:.1e} (bound {tol_cls(n):.1e}), reg {e_reg:.1e} (bound {tol_reg(n):.2e}), {n_idx}/{k} ranked '
          f'(query, class) indices differ (reference against itself: {noise}, eps_n / 2 = {eps / 2:.1e}), boxes {e_box:.1e} (bound {TOL_BOX:.0e})')
    assert e_cls < tol_cls(n)
    assert e_reg < tol_reg(n)
    assert k == len(g['labels']) == len(ref)
    # a rank may differ from the golden only across a gap the reference itself crosses (count within its own pairwise count, gap <= 2.5 x its
    # largest tie gap) or across a gap of at most eps_n / 2 (the largest the logit bound can close).  The gap crossed at rank i: the golden score
    # there against the golden score of the candidate the engine put there (from the golden's own last-layer logits, top max_num or not)
    gscore = torch.from_numpy(g['cls'][-1].reshape(-1)).sigmoid().numpy()
    by_noise = 0
    for i, v in enumerate(flat):
        if int(v) == int(ref[i]):
            continue
        crossed = abs(float(g['topk_scores'][i]) - float(gscore[int(v)]))
        if crossed <= eps / 2:
            continue
        by_noise += 1
        assert crossed <= 2.5 * gap, (i, int(v), crossed)
    assert by_noise <= noise
    # (tests/test_branch_depth_cpu.py holds every golden to at most 8 ranked scores with a neighbour within eps_n / 2)
    assert same_rank.sum() >= k - 8 - noise and e_box < TOL_BOX


# ---------------------------------------------------------------------------------------------------------- 5. engine consistency
@pytest.mark.parametrize('case,problem,n,dims', GOLDEN_CASES, ids=[c[0] for c in GOLDEN_CASES])
def test_engine_eager_graph_batch_fp16_and_last_stage(case, problem, n, dims):
    prob, prob2 = synthetic.make_problem(problem, seed=0), synthetic.make_problem(problem, seed=5)
    keys = ('cls', 'reg', 'boxes', 'scores', 'labels', 'bbox_index', 'count')
    eng = _engine(prob, n, dims)
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
    # two different frames through one sequence of launches
    single2 = {k: v.clone() for k, v in eng.run(feat2, props2, metas2).items() if k in keys}
    for use_graph in (False, True):
        ob = eng.run_batch([feat, feat2], [props, props2], [metas, metas2], use_graph=use_graph)
        grp = ob['grp_start'].tolist()
        assert torch.equal(ob['cls'][:, grp[0]:grp[1]], eager['cls']) and torch.equal(ob['reg'][:, grp[0]:grp[1]], eager['reg']), use_graph
        assert torch.equal(ob['cls'][:, grp[1]:grp[2]], single2['cls']) and torch.equal(ob['reg'][:, grp[1]:grp[2]], single2['reg']), use_graph
        for b, one in enumerate((eager, single2)):
            k_ = int(one['count'])
            assert int(ob['count'][b]) == k_
            for k in ('boxes', 'scores', 'labels'):
                assert torch.equal(ob[k][b, :k_], one[k][:k_]), (use_graph, b, k)
    # a 16-bit map: the same call on x.float()
    h = feat.half()
    o16, o32 = eng.run(h, props, metas), None
    got16 = {k: o16[k].clone() for k in keys}
    o32 = eng.run(h.float(), props, metas)
    for k in keys:
        assert torch.equal(got16[k], o32[k]), k
    # the last_stage_heads option evaluates the last layer only: the same last layer, the same detections
    last = _engine(prob, n, dims)
    last.last_stage_heads = True
    for use_graph in (False, True):
        o = last.run(feat, props, metas, use_graph=use_graph)
        assert torch.equal(o['cls'][-1], eager['cls'][-1]) and torch.equal(o['reg'][-1], eager['reg'][-1]), use_graph
        for k in ('boxes', 'scores', 'labels', 'count'):
            assert torch.equal(o[k], eager[k]), (use_graph, k)
    # the depth is checked against the state dict when the engine is built
    from mv2d_amd.engine import HeadEngine
    rl = dict(use_reg_layer=True, group_reg_dims=dims) if dims else {}
    with pytest.raises(ValueError, match='num_reg_fcs'):
        HeadEngine(_state(n, dims), prob['kind'], torch.device(DEV), num_views=prob['views_per_frame'], **rl)


def _per_layer_tables(sd, L, dims=None):
    """The tables of the per-layer entries (ops.heads_fused_x3 / heads_cls_x3 / reg_layer_x3: one [L] array per hidden layer) from a depth-2 state
    dict, packed as tests/test_gpu_branches_parent_bits.py packs them"""
    from mv2d_amd import ops
    t = lambda k: torch.as_tensor(sd['bbox_head.' + k]).float().to(DEV)
    st = lambda fmt: torch.stack([t(fmt.format(l)) for l in range(L)]).contiguous()
    c = {k: st('cls_branches.{}.' + k) for k in ('0.weight', '0.bias', '1.weight', '1.bias', '3.weight', '3.bias', '4.weight', '4.bias',
                                                 '6.weight', '6.bias')}
    cw = [*ops.pack_x3_stack(c['0.weight']), c['0.bias'], c['1.weight'], c['1.bias'], *ops.pack_x3_stack(c['3.weight']), c['3.bias'], c['4.weight'],
          c['4.bias'], c['6.weight'], c['6.bias']]
    if dims is None:
        r = {k: st('reg_branches.{}.' + k) for k in ('0.weight', '0.bias', '2.weight', '2.bias', '4.weight', '4.bias')}
        return cw, [*ops.pack_x3_stack(r['0.weight']), r['0.bias'], *ops.pack_x3_stack(r['2.weight']), r['2.bias'], r['4.weight'], r['4.bias']]
    sg = lambda fmt, join: torch.stack([join([t('reg_branches.' + fmt.format(l, g)) for g in range(len(dims))]) for l in range(L)]).contiguous()
    return cw, ops.pack_reg_layer(st('reg_branches.{}.reg_branch.0.weight'), st('reg_branches.{}.reg_branch.0.bias'),
                                  st('reg_branches.{}.reg_branch.3.weight'), st('reg_branches.{}.reg_branch.3.bias'),
                                  sg('{}.task_heads.{}.0.weight', torch.stack), sg('{}.task_heads.{}.0.bias', torch.stack),
                                  sg('{}.task_heads.{}.2.weight', torch.cat), sg('{}.task_heads.{}.2.bias', torch.cat))


def _assert_per_layer_entries_write_the_engines_bits(eng, out, sd):
    """The per-layer entries on the decoder outputs and reference points the finished run left in its workspace, with the rows, time steps and tables
    of the engine's own launch: cls and reg bit for bit the engine's (which launches the depth entries on [L][2] tables)."""
    from mv2d_amd import ops
    ws, R = out['ws'], out['R']
    L, M = ws['outs'].shape[:2]
    assert ws['cls'].shape[:2] == ws['reg'].shape[:2] == (L, M) and R <= M
    dims = eng.group_reg_dims if eng.use_reg_layer else None
    cw, rw = _per_layer_tables(sd, L, dims)
    cp, rp = ops.make_ptr_array(cw), ops.make_ptr_array(rw)
    cls, reg = torch.full_like(ws['cls'], SENTINEL), torch.full_like(ws['reg'], SENTINEL)
    dt_rows = ws['dt_rows'] if eng.kind == 'T' else None
    if dims is None:
        ops.heads_fused_x3(ws['outs'], cp, rp, ws['ref'], cls, reg, M, L, eng.pc_range_h, out['dt'], dt_rows=dt_rows, num_classes=eng.num_classes)
    else:
        ops.heads_cls_x3(ws['outs'], cp, cls, M, L, num_classes=eng.num_classes)
        ops.reg_layer_x3(ws['outs'], rp, ws['ref'], reg, M, L, dims, eng.pc_range_h, out['dt'], dt_rows=dt_rows)
    assert bool(torch.isfinite(out['cls']).all()) and bool(torch.isfinite(out['reg']).all())
    assert torch.equal(cls[:, :R], out['cls']) and torch.equal(reg[:, :R], out['reg'])


@pytest.mark.parametrize('problem', ['cfg1_s', 'cfg1_t'])
def test_engine_depth_2_is_the_engine_without_the_argument(problem):
    from mv2d_amd.engine import HeadEngine
    prob = synthetic.make_problem(problem, seed=0)
    sd = synthetic.make_head_state(seed=0)
    a = HeadEngine(sd, prob['kind'], torch.device(DEV), num_views=prob['views_per_frame'])
    b = HeadEngine(sd, prob['kind'], torch.device(DEV), num_views=prob['views_per_frame'], num_reg_fcs=2)
    assert a.num_reg_fcs == b.num_reg_fcs == 2
    # one table layout for every depth: both engines hold the same table keys, and the same tables
    assert set(a.w) == set(b.w) and 'head_tables' in a.w
    for ta, tb in zip(a.w['head_tables'], b.w['head_tables']):
        assert len(ta) == len(tb) and all(torch.equal(x, y) for x, y in zip(ta, tb))
    feat, props, metas = _inputs(prob)
    oa = {k: v.clone() for k, v in a.run(feat, props, metas).items() if torch.is_tensor(v)}
    ob = b.run(feat, props, metas)
    for k in ('cls', 'reg', 'boxes', 'scores', 'labels', 'bbox_index', 'count'):
        assert torch.equal(oa[k], ob[k]), k
    _assert_per_layer_entries_write_the_engines_bits(b, ob, sd)


def test_reg_layer_engine_writes_the_bits_of_the_per_layer_entries():
    """use_reg_layer at the shipped depth: the engine's class-only + RegLayer launches on stacked tables against heads_cls_x3 + reg_layer_x3"""
    prob = synthetic.make_problem('cfg1_s', seed=0)
    eng = _engine(prob, 2, DEFAULT)
    out = eng.run(*_inputs(prob))
    _assert_per_layer_entries_write_the_engines_bits(eng, out, _state(2, DEFAULT))


# ---------------------------------------------------------------------------------------------------------- 6. plugin head
def _build(kind, n, dims, use_denoise=None, train=False, num_views=2):
    import mv2d_amd
    cfg = (configs.roi_head_cfg_s if kind == 'S' else configs.roi_head_cfg_t)(num_reg_fcs=n, reg_layer_dims=dims)
    if kind == 'T':
        cfg['num_views'] = num_views                  # views per frame of the micro / cfg1 problems
    if use_denoise is not None:
        cfg['use_denoise'] = use_denoise
    head = mv2d_amd.build_head(cfg, train_cfg=configs.TRAIN_CFG_RCNN if train else None, test_cfg=configs.TEST_CFG_RCNN)
    sd = _state(n, dims) if (n != 2 or dims) else synthetic.make_head_state(seed=0)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=not train)
    return head.to(DEV)


@pytest.mark.parametrize('n,dims', [(1, None), (3, (2, 1, 3, 2, 2))], ids=['n1', 'n3_rl'])
def test_plugin_simple_test_equals_the_engine(n, dims):
    head = _build('S', n, dims).eval()
    probs = [synthetic.make_problem('cfg1_s', seed=s) for s in (0, 4)]
    feats = [torch.from_numpy(p['feat']).to(DEV) for p in probs]
    metas = [[dict(m, box_type_3d=None) for m in p['img_metas']] for p in probs]
    props = [[torch.from_numpy(x) for x in p['proposals']] for p in probs]
    singles = [head.simple_test([feats[b]], props[b], metas[b])[0] for b in range(2)]
    eng = _engine(probs[0], n, dims, max_num=300)
    out = eng.run(feats[0], props[0], probs[0]['img_metas'])
    for a, w in zip(singles[0], eng.results(out)):
        assert torch.equal(a, w)
    assert len(singles[0][2]) > 0
    got = head.simple_test_batch([torch.cat(feats, 0)], props, metas)
    for b in range(2):
        for a, w in zip(got[b], singles[b]):
            assert torch.equal(a, w), b
    # the bbox head's own forward (the reference's signature) walks the blocks by depth: on the engine's decoder outputs it returns the engine's
    # logits and box codes (fp32 linears against the split-precision launch: the bound of tests/test_gpu_reg_layer.py for this comparison; a
    # RegLayer runs through the same launch as the engine's: equal)
    o = eng.run(feats[0], props[0], probs[0]['img_metas'], keep_stages=True)
    R, bh = o['R'], head.bbox_head
    outs = o['ws']['outs'][:, :R].clone(memory_format=torch.contiguous_format)
    bh.transformer.forward = lambda *a, **k: (outs.view(outs.shape[0], R, 1, 256), None)      # (S path: one query per RoI sample)
    z = torch.zeros(R, 1, 256, 1, 1, device=DEV)
    cls, reg = bh(o['ws']['ref'][:R].view(R, 1, 3).clone(), z, None, z)
    e_cls, e_reg = relerr(cls.reshape(-1, R, 10), o['cls'][:, :R]), relerr(reg.reshape(-1, R, 10), o['reg'][:, :R])
    print(f'[branch_depth plugin] n={n} dims={dims}: forward vs engine cls {e_cls:.2e}, reg {e_reg:.2e} (bound 5e-5)')
    assert e_cls < 5e-5
    if dims:
        assert torch.equal(reg.reshape(-1, R, 10), o['reg'][:, :R])
    else:
        assert e_reg < 5e-5


# ---------------------------------------------------------------------------------------------------------- 7. training
def _dropout_off(head):
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    return head


def _branch_parameters(head):
    return {k: p for k, p in head.named_parameters() if '.cls_branches.' in k or '.reg_branches.' in k}


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('name,kind,with_dn', [('micro_s', 'S', False), ('micro_t', 'T', True)])
def test_forward_train_at_depth(name, kind, with_dn, n):
    dims = (2, 1, 3, 2, 2) if (kind == 'T') == (n == 1) else None        # a RegLayer on one S and one T case
    G, seed = 5, 31
    head = _dropout_off(_build(kind, n, dims, use_denoise=with_dn, train=True))
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
    assert set(losses) == set(fwd) and all(bool(torch.isfinite(v).all()) for v in losses.values())
    for k in fwd:      # the two routes agree (16-bit K / V on the autograd route only; the bound of tests/test_gpu_train.py for the two routes)
        assert abs(float(fwd[k]) - float(losses[k])) <= 5e-3 * max(abs(float(fwd[k])), 1e-2), (k, float(fwd[k]), float(losses[k]))
    sum(losses.values()).backward()
    params = _branch_parameters(head)
    from mv2d_amd.autograd_ops import branch_params
    want = {'bbox_head.' + p.format(l=l) for l in range(6) for p in branch_params(bool(dims), dims or (), n)}
    assert set(params) == want
    for k, p in params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k


def _branch_grad_errors(head, n, dims, T=77):
    """Gradients of sum(wc * logits) + sum(wb * box code) through TrainDecoder._branches against torch autograd on the fp64 restatement: the
    largest error per kind of quantity (relative to the largest entry of the fp64 gradient), for every branch parameter and the decoder outputs."""
    from mv2d_amd import train
    dec = train.TrainDecoder(head)
    L = dec.L
    outs = rnd((L, T, 256), 71).to(DEV).requires_grad_(True)
    ref = (torch.from_numpy(np.random.Generator(np.random.PCG64(72)).random((T, 3)).astype(np.float32)) * 0.9 + 0.05).to(DEV)
    wb, wc = rnd((L, T, 10), 73).to(DEV), rnd((L, T, 10), 74).to(DEV)
    head.zero_grad(set_to_none=True)
    cls, box = dec._branches(outs, ref, 0, 0.0)
    ((box * wb).sum() + (cls * wc).sum()).backward()
    P = {k[len('bbox_head.'):]: p for k, p in _branch_parameters(head).items()}
    P64 = {k: p.detach().double().cpu().requires_grad_(True) for k, p in P.items()}
    o64 = outs.detach().double().cpu().requires_grad_(True)
    raw = reg_layer_raw(P64, o64, n, dims) if dims else seq_raw(P64, o64, n)
    cls64, box64 = cls_raw(P64, o64, n), box_code(raw, ref.double().cpu())
    errs = {'fwd': max(relerr(box, box64), relerr(cls, cls64))}
    ((box64 * wb.double().cpu()).sum() + (cls64 * wc.double().cpu()).sum()).backward()

    def kind(k, p):
        if p.dim() == 2:
            return 'w256' if tuple(p.shape) == (256, 256) else 'w_out'
        w = P[k[:-len('bias')] + 'weight'] if k.endswith('bias') else None
        if w is None or w.dim() == 1:                                   # LayerNorm weight / bias
            return 'ln_w' if w is None else 'ln_b'
        return 'b256' if tuple(w.shape) == (256, 256) else 'b_out'
    for k, g, w in [('d_outs', outs.grad, o64.grad)] + [(k, P[k].grad, P64[k].grad) for k in P]:
        assert g is not None and bool(torch.isfinite(g).all()), k
        kk = k if k == 'd_outs' else kind(k, P[k])
        errs[kk] = max(errs.get(kk, 0.0), relerr(g, w))
    return errs


@functools.lru_cache(maxsize=None)
def _shipped_grad_errors():
    return _branch_grad_errors(_dropout_off(_build('S', 2, None, train=True)), 2, None)


@pytest.mark.parametrize('n,dims', [(1, None), (3, None), (1, DEFAULT), (3, (2, 1, 3, 2, 2))], ids=['n1', 'n3', 'n1_rl', 'n3_rl'])
def test_branch_gradients_match_fp64_autograd(n, dims):
    """The bound of tests/test_gpu_reg_layer.py's gradient test: the same heads-only function through the shipped HeadsFn node (depth 2) and
    through the per-operator nodes of the other depths, each against torch autograd on its fp64 restatement; the per-operator route may show
    twice the shipped route's error for every kind of quantity."""
    shipped = _shipped_grad_errors()
    new = _branch_grad_errors(_dropout_off(_build('S', n, dims, train=True)), n, dims)
    print('[branch_depth grads] shipped HeadsFn vs fp64:    ' + ', '.join(f'{k} {v:.2e}' for k, v in sorted(shipped.items())))
    print(f'[branch_depth grads] n={n} dims={dims} vs fp64: ' + ', '.join(f'{k} {v:.2e}' for k, v in sorted(new.items())))
    assert set(new) == set(shipped) == {'fwd', 'd_outs', 'w256', 'b256', 'w_out', 'b_out', 'ln_w', 'ln_b'}
    for k in new:
        assert new[k] <= 2.0 * shipped[k], (k, new[k], shipped[k])
