"""Class counts other than nuScenes' 10 on the GPU (-m gpu): the class output layer of the fused prediction branches
(mv2d_heads_fused_x3_nc), the top-k decode above 16384 candidates (the streamed variant of mv2d_decode_topk), the engine against goldens of the
unmodified reference built with num_classes = N (tests/golden/ncls_*.npz, tools/gen_golden_num_classes.py), the plugin head and both
training routes."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden, unpack_bits
from mv2d_amd import configs, synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -12345.0


def relerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def rnd(shape, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------- 1. prediction branches
def _branch_ptrs(sdt, L):
    from mv2d_amd import ops
    st = lambda fmt: torch.stack([sdt[fmt.format(l)] for l in range(L)]).contiguous().to(DEV)
    c = {n: st('bbox_head.cls_branches.{}.' + n) for n in ('0.weight', '0.bias', '1.weight', '1.bias', '3.weight', '3.bias', '4.weight', '4.bias',
                                                         '6.weight', '6.bias')}
    r = {n: st('bbox_head.reg_branches.{}.' + n) for n in ('0.weight', '0.bias', '2.weight', '2.bias', '4.weight', '4.bias')}
    cw = [*ops.pack_x3_stack(c['0.weight']), c['0.bias'], c['1.weight'], c['1.bias'], *ops.pack_x3_stack(c['3.weight']), c['3.bias'], c['4.weight'],
          c['4.bias'], c['6.weight'], c['6.bias']]
    rw = [*ops.pack_x3_stack(r['0.weight']), r['0.bias'], *ops.pack_x3_stack(r['2.weight']), r['2.bias'], r['4.weight'], r['4.bias']]
    return cw, rw


def _guarded(n, guard=4096):
    buf = torch.full((n + guard,), SENTINEL, device=DEV)
    return buf, buf[:n]


@pytest.mark.parametrize('M', [77, 531, 1100])                   # RT = 1, 2, 4 row tiles per block
@pytest.mark.parametrize('N', [1, 3, 10, 16, 17, 26, 64])
def test_heads_fused_x3_num_classes(N, M):
    from mv2d_amd import _lib, ops
    from oracle import mv2d_oracle as O
    sdt = {k: torch.from_numpy(v) for k, v in synthetic.make_head_state(seed=0, num_classes=N).items()}
    L = 6
    outs = rnd((L, M, 256), 51)
    ref = torch.from_numpy(np.random.Generator(np.random.PCG64(52)).random((M, 3)).astype(np.float32)) * 1.4 - 0.2
    cls_ref, reg_ref = O.pred_heads(sdt, outs, ref)
    dt_rows = torch.where(torch.arange(M) < 40, 0.5, 0.25).float()
    reg_ref = torch.cat([reg_ref[..., :8], reg_ref[..., 8:] / dt_rows[None, :, None]], -1)
    cw, rw = _branch_ptrs(sdt, L)
    cp, rp = ops.make_ptr_array(cw), ops.make_ptr_array(rw)
    cls_buf, cls_flat = _guarded(L * M * N)
    reg_buf, reg_flat = _guarded(L * M * 10)
    cls, reg = cls_flat.view(L, M, N), reg_flat.view(L, M, 10)
    pcr = torch.tensor(O.PC_RANGE, dtype=torch.float32)
    outs_d, ref_d, dtr_d = outs.to(DEV), ref.to(DEV), dt_rows.to(DEV)
    rc = _lib.load().mv2d_heads_fused_x3_nc(outs_d.data_ptr(), cp, rp, ref_d.data_ptr(), cls.data_ptr(), reg.data_ptr(), M, L, N, ctypes.c_float(1e-5),
                                            pcr.data_ptr(), ctypes.c_float(123.0), dtr_d.data_ptr(), ops._stream())
    assert rc == 0, _lib.load().mv2d_last_error()
    torch.cuda.synchronize()
    assert cls.shape == cls_ref.shape
    assert relerr(cls, cls_ref) < 5e-5
    assert relerr(reg, reg_ref) < 5e-5
    assert bool((cls_buf[L * M * N:] == SENTINEL).all()) and bool((reg_buf[L * M * 10:] == SENTINEL).all())      # nothing written past [L, M, N]
    # the keyword of the Python wrapper reaches the same entry
    cls2 = torch.empty((L, M, N), device=DEV); reg2 = torch.empty((L, M, 10), device=DEV)
    ops.heads_fused_x3(outs_d, cp, rp, ref_d, cls2, reg2, M, L, pcr, dt=123.0, dt_rows=dtr_d, num_classes=N)
    assert torch.equal(cls2, cls) and torch.equal(reg2, reg)
    if N == 10:
        # the 10-class entry point computes bitwise what the class-generic one computes
        cls3 = torch.empty((L, M, 10), device=DEV); reg3 = torch.empty((L, M, 10), device=DEV)
        rc = _lib.load().mv2d_heads_fused_x3(outs_d.data_ptr(), cp, rp, ref_d.data_ptr(), cls3.data_ptr(), reg3.data_ptr(), M, L, ctypes.c_float(1e-5),
                                             pcr.data_ptr(), ctypes.c_float(123.0), dtr_d.data_ptr(), ops._stream())
        assert rc == 0
        assert torch.equal(cls3, cls) and torch.equal(reg3, reg)


def test_heads_fused_x3_rejects_class_counts_outside_1_64():
    from mv2d_amd import ops
    with pytest.raises(ValueError, match='64'):
        ops.heads_fused_x3(None, None, None, None, None, None, 16, 6, torch.zeros(6), num_classes=65)
    with pytest.raises(ValueError, match='64'):
        ops.heads_fused_x3(None, None, None, None, None, None, 16, 6, torch.zeros(6), num_classes=0)


# ---------------------------------------------------------------------------------------------------------- 2. top-k decode
def _decode(cls, reg, R, N, max_num=300, grp=None, max_rows=0):
    from mv2d_amd import ops
    from oracle import mv2d_oracle as O
    B = 1 if grp is None else grp.numel() - 1
    boxes = torch.zeros((B, max_num, 9), device=DEV); scores = torch.zeros((B, max_num), device=DEV)
    labels = torch.zeros((B, max_num), dtype=torch.int64, device=DEV); bidx = torch.zeros((B, max_num), dtype=torch.int64, device=DEV)
    cnt = torch.zeros(B, dtype=torch.int32, device=DEV)
    ops.decode_topk(cls.to(DEV).contiguous(), reg.to(DEV).contiguous(), R, N, max_num, torch.tensor(O.POST_RANGE, dtype=torch.float32), boxes, scores,
                    labels, bidx, cnt, grp_start=grp, max_grp_rows=max_rows)
    torch.cuda.synchronize()
    return boxes, scores, labels, bidx, cnt


def _cls_reg(R, N, seed):
    cls = rnd((R, N), seed, 2.0) - 3.0
    reg = rnd((R, 10), seed + 100)
    reg[:, 0] *= 40.0; reg[:, 1] *= 40.0; reg[:, 4] *= 6.0                         # some centres fall outside the range
    return cls, reg


@pytest.mark.parametrize('R,N', [(12, 1), (300, 3), (300, 64), (900, 26), (1024, 64)])     # the last three: above 16384 candidates
def test_decode_topk_num_classes(R, N):
    from oracle import mv2d_oracle as O
    cls, reg = _cls_reg(R, N, 90 + N)
    boxes, scores, labels, bidx, cnt = _decode(cls, reg, R, N)
    b_ref, s_ref, l_ref, i_ref = O.decode(cls, reg, num_classes=N)
    n = int(cnt[0])
    assert n == b_ref.shape[0]
    assert torch.equal(labels[0, :n].cpu(), l_ref) and torch.equal(bidx[0, :n].cpu(), i_ref)
    assert relerr(scores[0, :n], s_ref) < 1e-6
    assert relerr(boxes[0, :n], b_ref) < 1e-5


def test_decode_topk_tie_order_above_16384_candidates():
    R, N = 900, 26
    cls, reg = _cls_reg(R, N, 95)
    reg = reg * 0.1
    flat = cls.view(-1)
    for i in (22999, 7, 16500):                                                       # a three-way tie at the top, spread over the whole set
        flat[i] = 50.0                                                                # above every drawn logit
    boxes, scores, labels, bidx, cnt = _decode(cls, reg, R, N)
    assert int(cnt[0]) == 300
    got = (bidx[0, :3] * N + labels[0, :3]).cpu().tolist()
    assert got == [7, 16500, 22999]
    assert bool((scores[0, :299] >= scores[0, 1:300]).all())


def test_decode_topk_batched_mixed_sizes_equals_single_launches():
    N = 26
    ca, ra = _cls_reg(300, N, 97)
    cb, rb = _cls_reg(900, N, 98)
    grp = torch.tensor([0, 300, 1200], dtype=torch.int32, device=DEV)
    got = _decode(torch.cat([ca, cb]), torch.cat([ra, rb]), 1200, N, grp=grp, max_rows=900)
    for s, (c, r, R) in enumerate(((ca, ra, 300), (cb, rb, 900))):
        one = _decode(c, r, R, N)
        for a, w in zip(got, one):
            assert torch.equal(a[s], w[0]), s


# ---------------------------------------------------------------------------------------------------------- 3. engine vs reference goldens
CASES = [('cfg2_s', 3), ('cfg3_t', 1), ('cfg5_t', 26)]
_RN = load_golden('ncls_refnoise')


@pytest.mark.parametrize('name,N', CASES)
def test_engine_matches_reference_golden_num_classes(name, N):
    from mv2d_amd.engine import HeadEngine
    g = load_golden(f'ncls_{name}_n{N}')
    key = f'{name}_n{N}_s0'
    noise, gap = int(_RN[key + '_pairwise_ranked_diff'].max()), float(_RN[key + '_max_tie_gap'])
    prob = synthetic.make_problem(name, seed=0)
    eng = HeadEngine(synthetic.make_head_state(seed=0, num_classes=N), prob['kind'], torch.device(DEV), num_views=prob['views_per_frame'],
                     num_classes=N, exact=True)
    out = eng.run(torch.from_numpy(prob['feat']).to(DEV), [torch.from_numpy(np.asarray(p)) for p in prob['proposals']], prob['img_metas'],
                  keep_stages=True)
    torch.cuda.synchronize()
    R, st = out['R'], out['stages']
    assert out['cls'].shape == (eng.L, R, N)
    if prob['kind'] == 'T':
        # key list + allowed pairs: bit-exact against the reference's boolean masks (as tests/test_gpu_golden.py)
        ffr = unpack_bits(g['feat_for_rois'], g['feat_for_rois_shape'])
        roi_mask = ffr.any(0).reshape(-1)
        np.testing.assert_array_equal(st['roi_mask'].cpu().numpy().astype(bool), roi_mask)
        assert int(st['S_dev'].item()) == int(roi_mask.sum())
        allowed = ffr.reshape(R, -1)[:, roi_mask] & ~g['key_padding'][None]
        rp, ci = st['row_ptr'].cpu().numpy(), st['col_idx'].cpu().numpy()
        for r in range(R):
            np.testing.assert_array_equal(np.sort(ci[rp[r]:rp[r + 1]]), np.nonzero(allowed[r])[0])
    e_cls = relerr(out['cls'][:, :R].reshape(g['cls'].shape), g['cls'])
    assert e_cls < 3e-6, e_cls
    n = int(out['count'].item())
    labels = out['labels'][:n].cpu().numpy()
    assert n == len(g['labels']) and bool((labels < N).all()) and bool((labels >= 0).all())
    flat = out['bbox_index'][:n].cpu().numpy() * N + labels
    ref = g['topk_index']
    assert len(ref) == n
    n_idx = int((flat != ref).sum())
    print(f'[num_classes {N}] {name}: {n_idx}/{n} ranked (query, class) indices differ (reference against itself: {noise}), cls rel err {e_cls:.1e}')
    assert n_idx <= noise
    pos = {int(v): j for j, v in enumerate(ref)}
    for i, v in enumerate(flat):
        if int(v) != int(ref[i]):
            j = pos.get(int(v))
            assert j is not None and abs(float(g['topk_scores'][i]) - float(g['topk_scores'][j])) <= 2.5 * gap, (i, int(v))


# ---------------------------------------------------------------------------------------------------------- 4. plugin head
def _build(kind, N, use_denoise=None, train=False):
    import mv2d_amd
    cfg = configs.roi_head_cfg_s(num_classes=N) if kind == 'S' else configs.roi_head_cfg_t(num_classes=N)
    if use_denoise is not None:
        cfg['use_denoise'] = use_denoise
    head = mv2d_amd.build_head(cfg, train_cfg=configs.TRAIN_CFG_RCNN if train else None, test_cfg=configs.TEST_CFG_RCNN)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_head_state(seed=0, num_classes=N).items()}, strict=not train)
    return head.to(DEV)


def test_plugin_simple_test_num_classes_3():
    from mv2d_amd import postprocess
    from mv2d_amd.engine import HeadEngine
    N = 3
    head = _build('S', N).eval()
    probs = [synthetic.make_problem('cfg1_s', seed=s) for s in (0, 4)]
    feats = [torch.from_numpy(p['feat']).to(DEV) for p in probs]
    metas = [[dict(m, box_type_3d=None) for m in p['img_metas']] for p in probs]
    props = [[torch.from_numpy(x) for x in p['proposals']] for p in probs]
    singles = [head.simple_test([feats[b]], props[b], metas[b])[0] for b in range(2)]
    # the engine run of the same weights
    eng = HeadEngine(synthetic.make_head_state(seed=0, num_classes=N), 'S', torch.device(DEV), num_views=probs[0]['views_per_frame'],
                     max_num=300, num_classes=N)
    ref = eng.results(eng.run(feats[0], props[0], probs[0]['img_metas']))
    for a, w in zip(singles[0], ref):
        assert torch.equal(a, w)
    assert bool((singles[0][2] < N).all()) and len(singles[0][2]) > 0
    # two samples through one sequence of launches == the two single calls
    got = head.simple_test_batch([torch.cat(feats, 0)], props, metas)
    for b in range(2):
        for a, w in zip(got[b], singles[b]):
            assert torch.equal(a, w), b
    # post-NMS pack: class-major, every label one of the N classes
    boxes, scores, labels = singles[0]
    res = postprocess.pack_results(boxes.contiguous(), scores.contiguous(), labels.contiguous(),
                                   torch.tensor([len(labels)], dtype=torch.int32, device=DEV), 0.0, 300)
    lab = res['labels_3d']
    assert len(lab) == len(labels) and bool((lab < N).all()) and bool((lab[1:] >= lab[:-1]).all())
    # a graph-replayed second frame == an eager one
    e = head.engine(feats[0].device, metas[0])
    e.run(feats[0], props[0], metas[0], use_graph=True)
    o_g = e.run(feats[0], props[1], metas[1], use_graph=True)
    g_res = [t.clone() for t in e.results(o_g)]
    o_e = e.run(feats[0], props[1], metas[1])
    for a, w in zip(g_res, e.results(o_e)):
        assert torch.equal(a, w)


# ---------------------------------------------------------------------------------------------------------- 5. training, both routes
def _dropout_off(head):
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    return head


@pytest.mark.parametrize('with_dn', [False, True])
def test_forward_train_num_classes_3(with_dn):
    from mv2d_amd import train
    from oracle import mv2d_oracle as O
    N, G, seed = 3, 9, 31
    head = _dropout_off(_build('S', N, use_denoise=with_dn, train=True))
    prob = synthetic.make_problem('cfg1_s', seed=0)
    gtc = synthetic.make_train_gt(G, seed)
    gt_labels = torch.from_numpy(gtc['gt_labels'] % N)
    rnd_ = torch.from_numpy(synthetic.make_dn_noise(G * 10, seed)).to(DEV)
    feat = torch.from_numpy(prob['feat']).to(DEV)
    props = [torch.from_numpy(p) for p in prob['proposals']]
    metas = [dict(m, box_type_3d=None) for m in prob['img_metas']]
    gt_list = [torch.from_numpy(gtc['gt'])]
    hl = head._head_loss(torch.device('cuda', torch.cuda.current_device()))
    seen = {}
    orig_assign = hl.assigner.assign

    def record(*a, **k):
        seen['match'] = orig_assign(*a, **k)
        return seen['match']
    hl.assigner.assign = record
    with torch.no_grad():
        losses = head.forward_train([feat], metas, props, None, None, None, None, gt_list, [gt_labels], None, dn_noise=rnd_, autograd=False)
    hl.assigner.assign = orig_assign
    # the same head outputs through the oracle's loss_single / dn_loss_single with num_classes = 3 (times the stage weights)
    eng = head.engine(feat.device, metas)
    out = eng.run(feat, [p[:, :6] for p in props], metas)
    R, pad = out['R'], 0
    gt, lab = gt_list[0].to(DEV), gt_labels.to(DEV)
    if with_dn:
        padded, _, md = train.prepare_for_dn(out['ws']['ref'][:R], gt, lab, head.denoise_scalar, head.denoise_noise_scale, head.denoise_noise_trans,
                                             head.denoise_split, N, list(head.pc_range), rnd=rnd_, dense_mask=False)
        pad = md['pad_size']
        cls, reg = eng.train_forward(out, padded[0, :pad], md['dn_single'])
        known_labels, known_bboxs = md['known_lbs_bboxes']
        assert bool((known_labels <= N).all())
    else:
        cls, reg = eng.train_forward(out)
    assert cls.shape == (6, pad + R, N)
    sw = configs.TRAIN_CFG_RCNN['stage_loss_weights']
    cw = configs.roi_head_cfg_s()['bbox_head']['code_weights']
    match = seen['match'].long().cpu()
    want = {}
    for l in range(6):
        c_, b_ = cls[l, pad:].double().cpu(), reg[l, pad:].double().cpu()
        lc, lb, _ = O.loss_single(c_, b_, gt.double().cpu(), lab.cpu(), match=match[l], num_classes=N, code_weights=cw)
        want[f'l{l}.loss_cls'], want[f'l{l}.loss_bbox'] = float(lc) * sw[l], float(lb) * sw[l]
        if with_dn:
            dc, db = O.dn_loss_single(cls[l, :pad].double().cpu(), reg[l, :pad].double().cpu(), known_bboxs.double().cpu(), known_labels.cpu(), pad,
                                      head.denoise_split, num_classes=N, code_weights=cw, neg_bbox_loss=head.neg_bbox_loss)
            want[f'l{l}.dn_loss_cls'], want[f'l{l}.dn_loss_bbox'] = float(dc) * sw[l] * head.denoise_weight, float(db) * sw[l] * head.denoise_weight
    assert set(losses) == set(want), (sorted(losses), sorted(want))
    for k, v in want.items():
        assert abs(float(losses[k]) - v) <= 2e-3 * max(abs(v), 1e-2), (k, float(losses[k]), v)
    # the autograd route (same assignment: a near-tie of the Hungarian matching may flip under the rounding difference of the two routes)
    hl.assigner.assign = lambda *a, **k: seen['match']
    try:
        head.zero_grad(set_to_none=True)
        losses_ag = head.forward_train([feat], metas, props, None, None, None, None, gt_list, [gt_labels], None, dn_noise=rnd_, autograd=True)
    finally:
        hl.assigner.assign = orig_assign
    assert set(losses_ag) == set(want)
    for k, v in want.items():
        assert abs(float(losses_ag[k].detach()) - v) <= 2e-3 * max(abs(v), 1e-2), (k, float(losses_ag[k]), v)
    sum(losses_ag.values()).backward()
    for l in range(6):
        gw = head.bbox_head.cls_branches[l][6].weight.grad
        assert gw is not None and tuple(gw.shape) == (N, 256) and bool(torch.isfinite(gw).all()), l
