"""Query-generator shapes on the GPU (-m gpu): the cell-writing RoI conv in both precision forms and the pool-only kernel (csrc/roiconv_cells.hip)
against fp64, the flattened first fc through linear_x3, the engine against the reference goldens tests/golden/qg_shape_*.npz
(tools/gen_golden_qg_shape.py), its invariances at one non-shipped shape, the plugin head and module at one case and both forward_train routes at
the two training records (tools/gen_golden_qg_shape_train.py)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_golden, unpack_bits
from mv2d_amd import configs, qg_shape, synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# tests/test_gpu_roi_size.py::test_qg_conv_pool_roi_size: split precision against fp64 on the unrounded operands, key16 against fp64 on the rounded ones
TOL_X3, TOL_K16 = 2e-6, 1e-5
# tests/test_gpu_pe_depth.py::test_engine_matches_reference_golden_pe_depth
TOL_CENTER, TOL_CLS, TOL_BOX = 1.3e-4, 3e-6, 5e-3
K_FP32 = 8            # tests/test_gpu_xattn_lo.py: at most 8 x the error of a plain fp32 evaluation of the same operands
NAN = float('nan')
KEYS = json.load(open(os.path.join(GOLDEN, 'qg_shape_state_keys.json')))


def relerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def rnd(shape, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def pair_ok(hi, lo, v):
    """A stored hi + lo pair against the fp32 value: the bound of test_key16_conversion_rounds_to_nearest_and_saturates (fp16: 2^-21 relative over
    an absolute 2^-24), and the hi half is the value rounded once."""
    from mv2d_amd import ops
    assert torch.equal(hi, v.to(hi.dtype))
    if ops.key16_dtype() == torch.float16:
        err = (hi.double() + lo.double() - v.double()).abs()
        assert float((err - v.double().abs() * 2.0 ** -21).clamp_min(0).max()) <= 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------- 1. the cell-writing conv
_CONV = {}


def _conv_operands(layer=0):
    """Weight, bias, their packed forms and the key16-rounded weight of one conv layer: built once, shared by the cases, never written."""
    if layer not in _CONV:
        from mv2d_amd import ops
        wt = rnd((256, 256, 3, 3), 2500 + layer, 1.0 / 48)
        b = rnd((256,), 2600 + layer, 0.1)
        w2 = wt.permute(0, 2, 3, 1).reshape(256, 2304).contiguous().to(DEV)
        wr = ops.f32_to_key16(w2).float().cpu().reshape(256, 3, 3, 256).permute(0, 3, 1, 2)
        _CONV[layer] = dict(wt=wt, b=b, bd=b.to(DEV), wp=ops.pack_key16(w2), wx3=ops.pack_key16_x3(w2), wr=wr)
    return _CONV[layer]


def _conv_ref(x, wt, b, s):
    """float64 conv2d(3x3, padding 1) + ReLU; x [R,s*s,256] cell-major, wt [256,256,3,3] -> [R,s*s,256]."""
    R = x.shape[0]
    xi = x.double().reshape(R, s, s, 256).permute(0, 3, 1, 2)
    return F.relu(F.conv2d(xi, wt.double(), b.double(), padding=1)).permute(0, 2, 3, 1).reshape(R, s * s, 256)


def _run_cells(hi, lo, w, op, R, s, hi_out=True, lo_out=True, f32_out=True):
    """One launch into NaN buffers of R + 1 RoIs: (out_hi, out_lo, out_f32), None for an output that was not asked for."""
    from mv2d_amd import ops
    k16 = ops.key16_dtype()
    mk = lambda dt, on: torch.full((R + 1, s * s, 256), NAN, device=DEV, dtype=dt) if on else None      # noqa: E731
    oh, ol, of = mk(k16, hi_out), mk(k16, lo_out), mk(torch.float32, f32_out)
    ops.qg_conv_cells(hi, lo, w, op['bd'], out_hi=oh, out_lo=ol, out_f32=of, R=R, roi_size=s)
    for t in (oh, ol, of):
        if t is not None:
            assert bool(torch.isfinite(t[:R].float()).all()), 'every cell of the R RoIs is written'
            assert bool(torch.isnan(t[R:].float()).all()), 'nothing past row R * s * s'
    return oh, ol, of


# R = 1, 2, 3: one block per RoI at every s (there is no two-RoIs-per-block instance, so no pair tail to exercise): several blocks, and the
# rows behind the last RoI stay untouched; s: one valid tap | all-border cells | the resident shape (one chunk holds the RoI) | exactly one
# 64-cell chunk | the first two-chunk size | four chunks with the row window
@pytest.mark.parametrize('s', [1, 2, 7, 8, 9, 14])
@pytest.mark.parametrize('R', [1, 2, 3])
def test_conv_cells_against_fp64(R, s):
    from mv2d_amd import ops
    op = _conv_operands()
    x = rnd((R, s * s, 256), 2400 + s)
    xd = x.to(DEV)
    # split precision: fp64 on the unrounded operands
    hi, lo = ops.f32_to_key16(xd, with_lo=True)
    oh, ol, of = _run_cells(hi, lo, op['wx3'], op, R, s)
    e3 = relerr(of[:R], _conv_ref(x, op['wt'], op['b'], s))
    pair_ok(oh[:R], ol[:R], of[:R])
    # key16: fp64 on the rounded operands
    kh, kl, kf = _run_cells(hi, None, op['wp'], op, R, s)
    e16 = relerr(kf[:R], _conv_ref(hi.float().cpu(), op['wr'], op['b'], s))
    pair_ok(kh[:R], kl[:R], kf[:R])
    print(f'[conv_cells] R {R} s {s}: split precision rel err {e3:.2e} (bound {TOL_X3:.0e}), key16 rel err {e16:.2e} (bound {TOL_K16:.0e})')
    assert e3 < TOL_X3 and e16 < TOL_K16
    # each output alone: the same bits
    for (a, b_, w), want in (((hi, lo, op['wx3']), (oh, ol, of)), ((hi, None, op['wp']), (kh, kl, kf))):
        only_hi, _, _ = _run_cells(a, b_, w, op, R, s, lo_out=False, f32_out=False)
        _, _, only_f = _run_cells(a, b_, w, op, R, s, hi_out=False, lo_out=False)
        assert torch.equal(only_hi[:R].view(torch.int16), want[0][:R].view(torch.int16)) and torch.equal(only_f[:R], want[2][:R])


@pytest.mark.parametrize('s', [7, 9])
def test_conv_chain_layer_by_layer(s):
    """Two convs: layer 2 against the fp64 conv of the kernel's OWN stored layer-1 cells (the single-layer bounds apply unchanged), and the fused
    conv + pool launch that ends a pooled trunk against the fp64 mean of the same layer."""
    from mv2d_amd import ops
    R = 3
    op1, op2 = _conv_operands(0), _conv_operands(1)
    x = rnd((R, s * s, 256), 2700 + s)
    hi, lo = ops.f32_to_key16(x.to(DEV), with_lo=True)
    h1, l1, f1 = _run_cells(hi, lo, op1['wx3'], op1, R, s)
    assert relerr(f1[:R], _conv_ref(x, op1['wt'], op1['b'], s)) < TOL_X3
    _, _, f2 = _run_cells(h1[:R].contiguous(), l1[:R].contiguous(), op2['wx3'], op2, R, s)
    stored = (h1[:R].double() + l1[:R].double()).cpu()
    ref2 = _conv_ref(stored, op2['wt'], op2['b'], s)
    e2 = relerr(f2[:R], ref2)
    pooled = torch.full((R + 1, 256), NAN, device=DEV)
    ops.qg_conv_pool_x3(h1[:R].contiguous(), l1[:R].contiguous(), op2['wx3'], op2['bd'], pooled, R=R, roi_size=s)
    ep = relerr(pooled[:R], ref2.mean(1))
    # key16 form: layer 2 reads the hi rows alone
    k1, _, kf1 = _run_cells(hi, None, op1['wp'], op1, R, s, lo_out=False)
    assert relerr(kf1[:R], _conv_ref(hi.float().cpu(), op1['wr'], op1['b'], s)) < TOL_K16
    _, _, kf2 = _run_cells(k1[:R].contiguous(), None, op2['wp'], op2, R, s, hi_out=False, lo_out=False)
    ek = relerr(kf2[:R], _conv_ref(k1[:R].float().cpu(), op2['wr'], op2['b'], s))
    print(f'[conv_chain] s {s}: layer 2 split precision {e2:.2e}, fused pool {ep:.2e} (bound {TOL_X3:.0e}), key16 {ek:.2e} (bound {TOL_K16:.0e})')
    assert e2 < TOL_X3 and ep < TOL_X3 and ek < TOL_K16
    assert bool(torch.isnan(pooled[R:]).all())


# ---------------------------------------------------------------------------------------------------------- 2. pool only
@pytest.mark.parametrize('s', [1, 7, 14])
@pytest.mark.parametrize('R', [1, 3])
def test_avgpool_cells_against_fp64(R, s):
    from mv2d_amd import ops
    x = rnd((R, s * s, 256), 2800 + s)
    hi, lo = ops.f32_to_key16(x.to(DEV), with_lo=True)
    out = torch.full((R + 1, 272), NAN, device=DEV)                                  # a row pitch beyond 256: the columns behind stay untouched
    ops.avgpool_cells(hi, lo, out, R, s * s)
    e3 = relerr(out[:R, :256], x.double().mean(1))
    out16 = torch.full((R + 1, 256), NAN, device=DEV)
    ops.avgpool_cells(hi, None, out16, R, s * s)
    e16 = relerr(out16[:R], hi.double().mean(1))
    print(f'[avgpool_cells] R {R} s {s}: hi + lo rel err {e3:.2e}, hi rel err {e16:.2e} (bound {TOL_X3:.0e})')
    assert e3 < TOL_X3 and e16 < TOL_X3
    assert bool(torch.isnan(out[:R, 256:]).all()) and bool(torch.isnan(out[R:]).all()) and bool(torch.isnan(out16[R:]).all())
    # cells = 1: the fp32 copy of the hi + lo rows
    flat = torch.full((R * s * s + 1, 256), NAN, device=DEV)
    ops.avgpool_cells(hi, lo, flat, R * s * s, 1)
    assert torch.equal(flat[:-1], (hi.float() + lo.float()).view(-1, 256)) and bool(torch.isnan(flat[-1]).all())


# ---------------------------------------------------------------------------------------------------------- 3. the flattened fc
@pytest.mark.parametrize('K', [256 * 9, 256 * 49])
@pytest.mark.parametrize('R', [1, 33])
def test_flattened_fc_through_linear_x3(R, K):
    """The first shared fc of an un-pooled trunk (K = 256 s^2 at s = 3 and 7) on linear_x3 against fp64; allowed: K_FP32 x the error of a plain fp32
    evaluation (torch, CPU) of the same operands."""
    from mv2d_amd import ops
    N = 128
    A, W, b = rnd((R, K), 2900 + R), rnd((N, K), 2901, K ** -0.5), rnd((N,), 2902, 0.1)
    ref = torch.relu(A.double() @ W.double().T + b.double())
    yard = float((torch.relu(A @ W.T + b).double() - ref).abs().max())
    out = torch.full((R + 1, N), NAN, device=DEV)
    ops.linear_x3(A.to(DEV), ops.pack_x3(W.to(DEV)), b.to(DEV), N=N, K=K, act=1, out=out, M=R)
    err = float((out[:R].double().cpu() - ref).abs().max())
    print(f'[flat fc] R {R} K {K}: linear_x3 error {err:.3e} = {err / yard:.2f} x the fp32 evaluation ({yard:.3e})')
    assert err <= K_FP32 * yard
    assert bool(torch.isnan(out[R:]).all())


# ---------------------------------------------------------------------------------------------------------- 4. engine vs the reference goldens
GOLDEN_CASES = ['micro_s_c2', 'cfg1_t_c0_f2', 'cfg1_s_flat3', 'cfg1_t_enc']
_RN = load_golden('qg_shape_refnoise')


def _state(case):
    rec = KEYS[case]
    return synthetic.with_qg_shape_state(synthetic.make_head_state(seed=0), 0, rec['query_generator'], rec['roi_size'])


def _engine(prob, sd, keys, roi_size=7, **kw):
    from mv2d_amd.engine import HeadEngine
    return HeadEngine(sd, prob['kind'], torch.device(DEV), num_views=prob['views_per_frame'], roi_size=roi_size, query_generator=keys, **kw)


def _inputs(prob):
    return torch.from_numpy(prob['feat']).to(DEV), [torch.from_numpy(np.asarray(p)) for p in prob['proposals']], prob['img_metas']


def _same(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _ranks_vs_golden(flat, g, noise):
    ref = g['topk_index']
    assert len(ref) == len(flat)
    n_idx = int((flat != ref).sum())
    assert n_idx <= noise, (n_idx, noise)
    pos = {int(v): j for j, v in enumerate(ref)}
    for i, v in enumerate(flat):
        if int(v) != int(ref[i]):
            j = pos.get(int(v))
            assert j is not None and abs(float(g['topk_scores'][i]) - float(g['topk_scores'][j])) <= 1e-7, (i, int(v))
    return n_idx


@pytest.mark.parametrize('case', GOLDEN_CASES)
def test_engine_matches_reference_golden_qg_shape(case):
    """Every stage test_engine_matches_reference_golden_pe_depth compares, with its bounds; micro_s_c2 also the recorded per-conv outputs under the
    split-precision conv bound."""
    from mv2d_amd import ops
    g, rec = load_golden('qg_shape_' + case), KEYS[case]
    key = case + '_s0'
    noise, gap = int(_RN[key + '_pairwise_ranked_diff'].max()), float(_RN[key + '_max_tie_gap'])
    prob = synthetic.make_problem(rec['problem'], seed=0)
    s = rec['roi_size']
    eng = _engine(prob, _state(case), rec['query_generator'], s, exact=True)
    assert eng.qg == qg_shape.parse(rec['query_generator']) and not eng.qg.is_default
    out = eng.run(*_inputs(prob), keep_stages=True)
    torch.cuda.synchronize()
    R, st, ws = out['R'], out['stages'], out['ws']
    assert relerr(ws['intr'][:R, :16], g['intr']) < 1e-6
    if eng.qg.intrinsic:
        assert torch.equal(st['enc'][:R, eng.qg.fc_out:eng.qg.fc_out + 16], ws['intr'][:R, :16])
    assert not st['enc'][:R, eng.qg.enc_in:].any()                                    # the pad columns
    e_c, e_x = relerr(st['center'][:R], g['center_pred']), relerr(st['xyz'][:R], g['xyz'])
    print(f'[qg_shape] {case}: center rel err {e_c:.2e}, xyz rel err {e_x:.2e} (bound {TOL_CENTER:.1e})')
    if case == 'micro_s_c2':
        # conv 0: the cells the engine stored for conv 1 (hi + lo); conv 1: its cells and its fused pool, launched again on those stored cells
        h0, l0 = ws['qg_cells_hi0'][:R], ws['qg_cells_lo0'][:R]
        c0 = h0.double() + l0.double()
        rois0, rois1 = g['conv0_cell_rois'].astype(np.int64), g['conv1_cell_rois'].astype(np.int64)
        f1 = torch.empty((R, s * s, 256), device=DEV)
        wx3, b1 = eng.w['qg_convs'][1]
        ops.qg_conv_cells(h0.contiguous(), l0.contiguous(), wx3, b1, out_f32=f1, R=R, roi_size=s)
        p1 = torch.empty((R, 256), device=DEV)        # (the engine's pooled rows are gone: the decoder reuses that buffer; the same launch again)
        ops.qg_conv_pool_x3(h0.contiguous(), l0.contiguous(), wx3, b1, p1, R=R, roi_size=s)
        errs = dict(conv0_cells=relerr(c0[rois0], g['conv0_cells']), conv0_pooled=relerr(c0.mean(1), g['conv0_pooled']),
                    conv1_cells=relerr(f1[rois1], g['conv1_cells']), conv1_pooled=relerr(p1, g['conv1_pooled']))
        print(f'[qg_shape] {case}: per-conv outputs against the reference\'s fp32 record: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()) +
              f' (bound {TOL_X3:.0e})')
        assert max(errs.values()) < TOL_X3, errs
    assert e_c < TOL_CENTER and e_x < TOL_CENTER
    if prob['kind'] == 'T':
        ffr = unpack_bits(g['feat_for_rois'], g['feat_for_rois_shape'])
        roi_mask = ffr.any(0).reshape(-1)
        np.testing.assert_array_equal(st['roi_mask'].cpu().numpy().astype(bool), roi_mask)
        assert int(st['S_dev'].item()) == int(roi_mask.sum())
        allowed = ffr.reshape(R, -1)[:, roi_mask] & ~g['key_padding'][None]
        rp, ci = st['row_ptr'].cpu().numpy(), st['col_idx'].cpu().numpy()
        for r in range(R):
            np.testing.assert_array_equal(np.sort(ci[rp[r]:rp[r + 1]]), np.nonzero(allowed[r])[0])
    else:
        rp, ci = st['row_ptr'].cpu().numpy(), st['col_idx'].cpu().numpy()
        for r in range(R):
            ids = g['corr'][r][g['corr_mask'][r]]
            want = np.sort(np.concatenate([np.arange(s * s) + s * s * int(i) for i in ids]))
            np.testing.assert_array_equal(np.sort(ci[rp[r]:rp[r + 1]]), want)
    e_cls = relerr(out['cls'][:, :R].reshape(g['cls'].shape), g['cls'])
    n = int(out['count'].item())
    labels = out['labels'][:n].cpu().numpy()
    print(f'[qg_shape] {case}: cls rel err {e_cls:.2e} (bound {TOL_CLS:.0e}), reference against itself: {noise} ranked indices, gap {gap:.1e}')
    assert e_cls < TOL_CLS, e_cls
    assert n == len(g['labels'])
    n_idx = _ranks_vs_golden(out['bbox_index'][:n].cpu().numpy() * 10 + labels, g, noise)
    print(f'[qg_shape] {case}: {n_idx}/{n} ranked (query, class) indices differ')


# ---------------------------------------------------------------------------------------------------------- 5. engine invariances
# two convs (the cell-writing launch), two shared fcs of a width that is no multiple of 32 (the pad columns), a centre fc (fc_center off the row-fused kernel)
INV_KEYS = dict(num_shared_convs=2, num_shared_fcs=2, fc_out_channels=528, num_center_fcs=1)


@pytest.mark.parametrize('name', ['cfg1_s', 'cfg1_t'])
def test_engine_qg_shape_invariances(name):
    probs = [synthetic.make_problem(name, seed=s) for s in (0, 3, 5)]
    sd = synthetic.with_qg_shape_state(synthetic.make_head_state(seed=0), 0, INV_KEYS)
    eng = _engine(probs[0], sd, INV_KEYS)
    ins = [_inputs(p) for p in probs]
    singles = []
    for f, pr, m in ins:
        o = eng.run(f, pr, m)
        assert o['ws']['enc'].shape[1] == 544 and o['ws']['qg_shared_fcs_0'].shape[1] == 544 and 'qg_cells_hi0' in o['ws'] and 'qg_cells_hi1' not in o['ws']
        singles.append([t.clone() for t in eng.results(o)])
        assert len(singles[-1][2]) > 0 and bool(torch.isfinite(singles[-1][1]).all())
    # three samples through one sequence of launches == each sample alone
    ob = eng.run_batch([f for f, _, _ in ins], [pr for _, pr, _ in ins], [m for _, _, m in ins])
    for b in range(3):
        n = int(ob['count'][b])
        assert n == len(singles[b][2])
        _same((ob['boxes'][b, :n], ob['scores'][b, :n], ob['labels'][b, :n]), singles[b])
    # a graph-replayed frame == an eager one
    f, pr, m = ins[1]
    eng.run(f, ins[0][1], ins[0][2], use_graph=True)       # capture (other boxes), then a replay of sample 1's boxes
    og = eng.run(f, pr, m, use_graph=True)
    _same([t.clone() for t in eng.results(og)], singles[1])
    # an fp16 / bf16 map == the fp32 map holding the same values
    for dt in (torch.float16, torch.bfloat16):
        f16 = ins[0][0].to(dt)
        a = [t.clone() for t in eng.results(eng.run(f16, ins[0][1], ins[0][2]))]
        b = [t.clone() for t in eng.results(eng.run(f16.float(), ins[0][1], ins[0][2]))]
        _same(a, b)
    # one engine serving alternating RoI-count buckets
    few = [p[:max(1, len(p) // 5)] for p in ins[2][1]]
    fresh = _engine(probs[0], sd, INV_KEYS)
    want_few = [t.clone() for t in fresh.results(fresh.run(ins[2][0], few, ins[2][2]))]
    for _ in range(2):
        _same([t.clone() for t in eng.results(eng.run(ins[2][0], few, ins[2][2]))], want_few)
        _same([t.clone() for t in eng.results(eng.run(*ins[0]))], singles[0])


@pytest.mark.parametrize('name', ['cfg1_s', 'cfg1_t'])
def test_default_shape_written_out_gives_the_default_engines_bits(name):
    prob = synthetic.make_problem(name, seed=0)
    sd = synthetic.make_head_state(seed=0)
    explicit = dict(with_avg_pool=True, num_shared_convs=1, num_shared_fcs=1, num_center_fcs=0, fc_out_channels=1024,
                    extra_encoding=dict(num_layers=2, feat_channels=[512, 256], features=[dict(type='intrinsic', in_channels=16)]))
    outs = []
    for keys in (None, explicit):
        eng = _engine(prob, sd, keys)
        assert eng.qg.is_default and 'qg_lin' not in eng.w
        o = eng.run(*_inputs(prob))
        assert not any(k.startswith('qg_') for k in o['ws']) and tuple(o['ws']['enc'].shape[1:]) == (1056,)
        outs.append([t.clone() for t in eng.results(o)] + [o['cls'].clone(), o['reg'].clone()])
    _same(*outs)


def test_engine_qg_shape_refusals():
    """The key16 mode has no plan for other shapes: ValueError before any launch; a state dict of another shape is refused by parameter name."""
    prob = synthetic.make_problem('cfg1_t', seed=0)
    sd = synthetic.with_qg_shape_state(synthetic.make_head_state(seed=0), 0, INV_KEYS)
    with pytest.raises(ValueError, match='index-exact route only'):
        _engine(prob, sd, INV_KEYS, exact=False).run(*_inputs(prob))
    with pytest.raises(ValueError, match=r'HeadEngine: query_generator\.shared_fcs\.0\.weight is \(528, 256\)'):
        _engine(prob, sd, None)
    with pytest.raises(ValueError, match=r'HeadEngine: the state dict has no query_generator\.shared_convs\.1'):
        _engine(prob, synthetic.make_head_state(seed=0), dict(num_shared_convs=2))


# ---------------------------------------------------------------------------------------------------------- 6. plugin head and module
def _build(case, num_views, train=False):
    import mv2d_amd
    rec = KEYS[case]
    cfg = (configs.roi_head_cfg_s if rec['kind'] == 'S' else configs.roi_head_cfg_t)(query_generator=rec['query_generator'], roi_size=rec['roi_size'])
    if rec['kind'] == 'T':
        cfg['num_views'] = num_views
    head = mv2d_amd.build_head(cfg, train_cfg=configs.TRAIN_CFG_RCNN if train else None, test_cfg=configs.TEST_CFG_RCNN)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in _state(case).items()}, strict=not train)
    return head.to(DEV)


def test_plugin_simple_test_matches_golden_cfg1_t_c0_f2():
    """simple_test and simple_test_batch at num_shared_convs=0, num_shared_fcs=2, fc_out_channels=512, num_center_fcs=1: heads.py hands the module's
    shape to the engine; the module-level QueryGenerator.forward at the same shape against the golden's xyz."""
    case = 'cfg1_t_c0_f2'
    g = load_golden('qg_shape_' + case)
    noise = int(_RN[case + '_s0_pairwise_ranked_diff'].max())
    prob = synthetic.make_problem('cfg1_t', seed=0)
    head = _build(case, prob['views_per_frame']).eval()
    feat = torch.from_numpy(prob['feat']).to(DEV)
    metas = [dict(m, box_type_3d=None) for m in prob['img_metas']]
    props = [torch.from_numpy(x) for x in prob['proposals']]
    single = head.simple_test([feat], props, metas)[0]
    eng = head.engine(feat.device, metas)
    assert eng.qg == qg_shape.parse(KEYS[case]['query_generator'])
    batch = head.simple_test_batch([torch.cat([feat, feat], 0)], [props, props], [metas, metas])
    for b in range(2):
        _same(batch[b], single)
    boxes, scores, labels = (t.cpu().numpy() for t in single)
    n = len(labels)
    assert n == len(g['labels'])
    assert int((labels != g['labels']).sum()) <= noise
    assert float(np.abs(scores - g['scores']).max()) <= 0.25 * TOL_CLS * float(np.abs(g['cls']).max())
    same = labels == g['labels']
    assert float(np.abs(boxes - g['boxes'])[same].max() / np.abs(g['boxes']).max()) < TOL_BOX
    # the module's own forward on the engine's RoI cells (hi + lo), intrinsics rows and per-RoI cameras of the same frame
    out = eng.run(feat, props, metas, keep_stages=True)
    R, ws = out['R'], out['ws']
    x = (ws['roi_feat'][:R].float() + ws['roi_lo'][:R].float()).view(R, 7, 7, 256).permute(0, 3, 1, 2).contiguous()
    from oracle import mv2d_oracle as O
    st = {}
    O.forward_t(synthetic.make_head_state(seed=0), torch.from_numpy(prob['feat']), props, prob['img_metas'], num_views=prob['views_per_frame'], stages=st)
    xyz, _ = head.query_generator(x, st['K_roi'].to(DEV), st['E'].to(DEV), dict(intrinsic=ws['intr'][:R, :16].clone()))
    e = relerr(xyz, g['xyz'])
    print(f'[qg_shape] QueryGenerator.forward at {case}: xyz rel err {e:.2e} (bound {TOL_CENTER:.1e})')
    assert e < TOL_CENTER


# ---------------------------------------------------------------------------------------------------------- 7. training
def _dropout_off(head):
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    return head


@pytest.mark.parametrize('name,case', [('train_micro_s', 'micro_s_c2'), ('train_cfg1_t', 'cfg1_t_c0_f2')])
def test_forward_train_qg_shape_matches_reference(name, case):
    """Both forward_train routes at the two training records against each other (2e-3 * max(|v|, 1e-2)) and against the reference's own record
    under the comparison of test_forward_train_depth_32_matches_reference; every parameter of the shape gets a gradient of the module's own shape."""
    gold = load_golden('qg_shape_train')
    prob_name, kind, G, seed = synthetic.FWD_TRAIN_CASES[name]
    prob = synthetic.make_problem(prob_name, seed=0)
    head = _dropout_off(_build(case, prob['views_per_frame'], train=True))
    gtc = synthetic.make_train_gt(G, seed)
    rnd_ = torch.from_numpy(synthetic.make_dn_noise(G * 10, seed)).to(DEV)
    feat = torch.from_numpy(prob['feat']).to(DEV).requires_grad_(True)
    props = [torch.from_numpy(p) for p in prob['proposals']]
    metas = [dict(m, box_type_3d=None) for m in prob['img_metas']]
    gt_list, lab_list = [torch.from_numpy(gtc['gt'])], [torch.from_numpy(gtc['gt_labels'])]
    hl = head._head_loss(torch.device('cuda', torch.cuda.current_device()))
    want_match = torch.from_numpy(gold[name + '.match']).to(DEV)
    orig_assign = hl.assigner.assign
    hl.assigner.assign = lambda *a, **k: want_match           # the reference's assignment (a near-tie may flip under rounding)
    try:
        with torch.no_grad():
            losses_f = head.forward_train([feat], metas, props, None, None, None, None, gt_list, lab_list, None, dn_noise=rnd_, autograd=False)
        head.zero_grad(set_to_none=True)
        losses = head.forward_train([feat], metas, props, None, None, None, None, gt_list, lab_list, None, dn_noise=rnd_, autograd=True)
    finally:
        hl.assigner.assign = orig_assign
    assert set(losses) == set(losses_f)
    for k in losses_f:                                         # the two routes agree
        v = float(losses_f[k])
        assert np.isfinite(v) and abs(float(losses[k].detach()) - v) <= 2e-3 * max(abs(v), 1e-2), (k, float(losses[k]), v)
    for got in (losses_f, losses):                             # ... and match the reference
        assert set(got) == {k[len(name) + 6:] for k in gold if k.startswith(name + '.loss.')}
        for k in got:
            v = float(gold[f'{name}.loss.{k}'])
            assert abs(float(got[k].detach()) - v) <= 2e-3 * max(abs(v), 1e-2), (k, float(got[k].detach()), v)
    sum(losses.values()).backward()
    params = dict(head.named_parameters())
    names = [str(n) for n in gold[name + '.grad_names']]
    for k, shp in KEYS[case]['params'].items():                # every parameter of the shape: a gradient of the module's own shape
        p = params['query_generator.' + k]
        assert 'query_generator.' + k in names and p.grad is not None and list(p.grad.shape) == shp == list(p.shape), k
    worst, errs, top = (0.0, None), [], float(gold[name + '.grad_norm'].max())
    for n, norm, proj in zip(names, gold[name + '.grad_norm'], gold[name + '.grad_proj']):
        gr = params[n].grad
        assert gr is not None, n
        if norm < 1e-5 * top:
            continue
        gr = gr.double().cpu()
        got_norm = float(gr.norm())
        got_proj = float((gr.flatten() * torch.from_numpy(synthetic.grad_probe(n, gr.numel())).double()).sum())
        e = max(abs(got_norm - norm), abs(got_proj - proj) / 3.0) / norm
        if n.startswith('query_generator.') and n.endswith('weight'):
            print(f'[qg_shape train] {name}: {n} grad norm {got_norm:.4e} (reference {norm:.4e}), rel err {e:.2e}')
        errs.append(e)
        if e > worst[0]:
            worst = (e, n)
    gf = feat.grad.double().cpu()
    fn = float(gold[name + '.dfeat_norm'])
    assert abs(float(gf.norm()) - fn) <= 2e-2 * fn
    assert torch.allclose(gf.flatten(1).norm(dim=1), torch.from_numpy(gold[name + '.dfeat_view_norms']), rtol=3e-2, atol=1e-3 * fn)
    errs.sort()
    assert worst[0] <= 0.15 and errs[len(errs) // 2] <= 1e-2, (worst, errs[len(errs) // 2])
