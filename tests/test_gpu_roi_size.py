"""RoI sizes other than 7 on the GPU (-m gpu): the size-taking kernels over s = 1 .. 14 (RoIAlign forward / backward, the RoIAlign tap cells
and the S-path key lists, the query generator's conv + pool in both precisions, im2col / col2im), the engine's invariances at s = 5
(batch == single samples, graph replay == eager, key16 and fp16 lo rows, s = 7 passed explicitly == the default), the engine against goldens of
the unmodified reference built with roi_size = s (tests/golden/roi_size_*.npz, tools/gen_golden_roi_size*.py), the plugin head and both
training routes against the reference's training record at s = 5."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, unpack_bits
from mv2d_amd import configs, synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = list(range(1, 15))


def relerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def rnd(shape, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def _rois(V, h, w, seed):
    """RoIs in pixels (stride 16): ordinary ones, ones across every map border, tiny (< 1 cell) and huge (larger than the map) ones."""
    g = np.random.Generator(np.random.PCG64(seed))
    W_, H_ = 16.0 * w, 16.0 * h
    out = []
    for _ in range(24):
        x1, y1 = g.uniform(0, W_ - 40), g.uniform(0, H_ - 40)
        out.append([x1, y1, x1 + g.uniform(8, 300), y1 + g.uniform(8, 200)])
    out += [[-50.0, -30.0, 120.0, 90.0], [W_ - 100, H_ - 60, W_ + 80, H_ + 40], [-200.0, 10.0, -5.0, 100.0], [3.0, 4.0, 9.0, 7.0],
            [100.0, 100.0, 100.5, 100.25], [-300.0, -300.0, W_ + 300, H_ + 300], [0.0, 0.0, W_, H_]]
    r = np.asarray(out, np.float32)
    v = g.integers(0, V, len(r)).astype(np.float32)
    return torch.from_numpy(np.concatenate([v[:, None], r], 1))


# ---------------------------------------------------------------------------------------------------------- 1. RoIAlign
@pytest.mark.parametrize('s', SIZES)
def test_roi_align_forward_roi_size(s):
    from mv2d_amd import ops
    from oracle import mv2d_oracle as O
    V, h, w = 2, 12, 20
    f0, f1 = rnd((V, 256, h, w), 10 + s), rnd((V, 256, h, w), 40 + s)
    rois = _rois(V, h, w, s)
    R = rois.shape[0]
    want0 = O.roi_align(f0, rois, out_size=s).permute(0, 2, 3, 1).reshape(R, s * s, 256)
    want1 = O.roi_align(f1, rois, out_size=s).permute(0, 2, 3, 1).reshape(R, s * s, 256)
    m0 = f0.permute(0, 2, 3, 1).reshape(-1, 256).contiguous().to(DEV)
    full1 = f1.permute(0, 2, 3, 1).reshape(-1, 256).contiguous()
    # map1 as a compacted map: row index[position] (a permutation of the positions)
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(s)).permutation(full1.shape[0]))
    comp = full1[perm].contiguous().to(DEV)
    index = torch.empty(full1.shape[0], dtype=torch.int32)
    index[perm] = torch.arange(full1.shape[0], dtype=torch.int32)
    rd = rois.to(DEV)
    o0 = torch.empty((R, s * s, 256), device=DEV)
    o1 = torch.empty_like(o0)
    k0 = torch.empty((R, s * s, 256), device=DEV, dtype=ops.key16_dtype())
    ops.roi_align(m0, rd, h, w, map1=comp, map1_index=index.to(DEV), out0=k0, out0_f32=o0, out1_f32=o1, R=R, roi_size=s)
    torch.cuda.synchronize()
    assert relerr(o0, want0) < 1e-6
    assert relerr(o1, want1) < 1e-6
    assert torch.equal(k0, ops.f32_to_key16(o0))           # the key16 output is the rounded fp32 output
    if s == 7:                                              # the 7x7 entry and the size-taking one agree bit for bit
        from mv2d_amd import _lib
        o7 = torch.empty_like(o0)
        # (mv2d_roi_align_ex through the library itself: ops.roi_align calls mv2d_roi_align_fmt for every size)
        _lib.check(_lib.load().mv2d_roi_align_ex(m0.data_ptr(), None, rd.data_ptr(), None, None, o7.data_ptr(), None, R, h, w, 256, 1.0 / 16, -1, None, 0,
                                                 None, None, None, None, None, ops._stream()), 'mv2d_roi_align_ex')
        assert torch.equal(o7, o0)
        od = torch.empty_like(o0)
        ops.roi_align(m0, rd, h, w, out0_f32=od, R=R)       # roi_size left at its default
        assert torch.equal(od, o0)


@pytest.mark.parametrize('s', [1, 2, 5, 9, 14])
def test_roi_align_backward_roi_size(s):
    from mv2d_amd import ops
    from oracle import mv2d_oracle as O
    V, h, w = 2, 10, 14
    f = rnd((V, 256, h, w), 70 + s).requires_grad_(True)
    rois = _rois(V, h, w, 90 + s)[:12]
    R = rois.shape[0]
    g = rnd((R, s * s, 256), 110 + s)
    O.roi_align(f, rois, out_size=s).permute(0, 2, 3, 1).reshape(R, s * s, 256).backward(g)
    rows = f.detach().permute(0, 2, 3, 1).reshape(-1, 256).contiguous().to(DEV).requires_grad_(True)
    out = ops.RoIAlignRows.apply(rows, None, rois.to(DEV), h, w, None, s)
    assert out.shape == (R, s * s, 256)
    out.backward(g.to(DEV))
    want = f.grad.permute(0, 2, 3, 1).reshape(-1, 256)
    assert relerr(rows.grad, want) < 1e-5


# ---------------------------------------------------------------------------------------------------------- 2. S-path tap cells and key lists
def _taps(lo_px, hi_px, n, s):
    """The cells the bilinear taps of an s-bin RoIAlign axis touch, every bin and every sample enumerated (as the 7x7 check in
    test_gpu_kernels.py): fp32 sample coordinates of mmcv's aligned, adaptive grid; taps (int) max(x, 0) and its neighbour, clamped."""
    f = np.float32
    a, b = f(f(lo_px) * f(0.0625) - f(0.5)), f(f(hi_px) * f(0.0625) - f(0.5))
    ln = f(b - a)
    bn = f(ln / f(s))
    gr = int(np.ceil(f(ln / f(s))))
    touched = set()
    for pw in range(s):
        for ix in range(gr):
            xx = f(f(a + f(f(pw) * bn)) + f(f(f(ix + 0.5) * bn) / f(gr)))
            if xx < -1.0 or xx > n:
                continue
            x = max(float(xx), 0.0)
            xl = int(x)
            if xl >= n - 1:
                xl = xh = n - 1
            else:
                xh = xl + 1
            touched.update((xl, xh))
    return touched


@pytest.mark.parametrize('s', SIZES)
def test_tap_cells_and_csr_roi_size(s):
    from mv2d_amd import ops
    V, h, w, topk = 3, 12, 20, 2
    rois = _rois(V, h, w, 200 + s)
    R = rois.shape[0]
    P = V * h * w
    g = np.random.Generator(np.random.PCG64(300 + s))
    match = np.where(g.uniform(size=(R, V, topk)) < 0.3, g.integers(0, R, (R, V, topk)), -1).astype(np.int32)
    pad_mask = torch.zeros(P, dtype=torch.uint8)
    z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=DEV)
    roi_mask, rect, pos2s, s2pos, S_dev = z(P, torch.uint8), z(R * 5), z(P), z(P), z(1)
    row_ptr, nnz = z(R + 1), z(2)
    col_idx = torch.full((R * (1 + V * topk) * s * s,), -7, dtype=torch.int32, device=DEV)
    ops.roi_positions_csr(rois.to(DEV), pad_mask.to(DEV), roi_mask, rect, pos2s, s2pos, S_dev, R, V, h, w, torch.from_numpy(match).to(DEV),
                          row_ptr, col_idx, nnz, V, topk, stride=16.0, expand_stride=-1.0, roi_size=s)
    torch.cuda.synchronize()
    # the cells every tap of the s x s RoIAlign touches
    want_mask = np.zeros((V, h, w), np.uint8)
    rn = rois.numpy()
    rc = rect.view(R, 5).cpu().numpy()
    for r in range(R):
        tx, ty = _taps(rn[r, 1], rn[r, 3], w, s), _taps(rn[r, 2], rn[r, 4], h, s)
        assert rc[r, 0] == int(rn[r, 0])
        if tx and ty:
            assert tuple(rc[r, 1:]) == (min(ty), max(ty), min(tx), max(tx)), (r, rn[r], rc[r])
            want_mask[int(rn[r, 0]), min(ty):max(ty) + 1, min(tx):max(tx) + 1] = 1
        else:
            assert rc[r, 2] < rc[r, 1] or rc[r, 4] < rc[r, 3], (r, rn[r], rc[r])
    np.testing.assert_array_equal(roi_mask.cpu().numpy(), want_mask.reshape(-1))
    assert int(S_dev.item()) == int(want_mask.sum())
    # key lists: s*s consecutive cells of the row's own RoI, then of each listed RoI in (view, rank) order
    rp, cols = [0], []
    for r in range(R):
        ids = [r] + [int(m) for m in match[r].reshape(-1) if m >= 0]
        for i in ids:
            cols += list(range(i * s * s, (i + 1) * s * s))
        rp.append(len(cols))
    np.testing.assert_array_equal(row_ptr.cpu().numpy(), np.asarray(rp, np.int32))
    np.testing.assert_array_equal(col_idx[:len(cols)].cpu().numpy(), np.asarray(cols, np.int32))
    assert int(nnz[0]) == len(cols)
    # the stand-alone CSR entry writes the same lists
    rp2, ci2, nz2 = z(R + 1), torch.full_like(col_idx, -7), z(2)
    ops.csr_from_corr(torch.from_numpy(match).to(DEV), rp2, ci2, nz2, R, V, topk, roi_size=s)
    assert torch.equal(rp2, row_ptr) and torch.equal(ci2, col_idx)


# ---------------------------------------------------------------------------------------------------------- 3. conv + pool, im2col
def _conv_pool_ref(x, wt, b, s):
    """float64 conv2d(3x3, padding 1) + ReLU + avg_pool2d(s); x [R,s*s,256] cell-major, wt [256,256,3,3]."""
    R = x.shape[0]
    xi = x.double().reshape(R, s, s, 256).permute(0, 3, 1, 2)
    return F.avg_pool2d(F.relu(F.conv2d(xi, wt.double(), b.double(), padding=1)), s).reshape(R, 256)


@pytest.mark.parametrize('s', SIZES)
def test_qg_conv_pool_roi_size(s):
    from mv2d_amd import ops
    R = 37
    x = rnd((R, s * s, 256), 400 + s)
    wt = rnd((256, 256, 3, 3), 500 + s, 1.0 / 48)
    b = rnd((256,), 600 + s, 0.1)
    w2 = wt.permute(0, 2, 3, 1).reshape(256, 2304).contiguous().to(DEV)
    xd = x.to(DEV)
    # key16 x key16: against the float64 composition on the rounded operands
    xh = ops.f32_to_key16(xd)
    out = torch.full((R, 256), float('nan'), device=DEV)
    ops.qg_conv_pool(xh, ops.pack_key16(w2), b.to(DEV), out, R=R, roi_size=s)
    wr = ops.f32_to_key16(w2).float().cpu().reshape(256, 3, 3, 256).permute(0, 3, 1, 2)
    assert relerr(out, _conv_pool_ref(xh.float().cpu(), wr, b, s)) < 1e-5
    # split precision (hi + lo cells and weights): against the float64 composition on the fp32 operands
    hi, lo = ops.f32_to_key16(xd, with_lo=True)
    out3 = torch.full((R, 256), float('nan'), device=DEV)
    ops.qg_conv_pool_x3(hi, lo, ops.pack_key16_x3(w2), b.to(DEV), out3, R=R, roi_size=s)
    assert relerr(out3, _conv_pool_ref(x, wt, b, s)) < 2e-6


@pytest.mark.parametrize('s', SIZES)
def test_im2col_col2im_roi_size(s):
    from mv2d_amd.autograd_ops import Im2Col3x3Fn
    R = 5
    x = rnd((R, s * s, 256), 700 + s)
    xi = x.reshape(R, s, s, 256).permute(0, 3, 1, 2).requires_grad_(True)
    want = F.unfold(xi, 3, padding=1).reshape(R, 256, 9, s * s).permute(0, 3, 2, 1).reshape(R * s * s, 2304)      # (cell, tap, channel)
    xd = x.to(DEV).requires_grad_(True)
    cols = Im2Col3x3Fn.apply(xd, s)
    assert torch.equal(cols.cpu(), want.detach())
    g = rnd((R * s * s, 2304), 800 + s)
    cols.backward(g.to(DEV))
    want.backward(g)
    assert relerr(xd.grad, xi.grad.permute(0, 2, 3, 1).reshape(R, s * s, 256)) < 1e-6


# ---------------------------------------------------------------------------------------------------------- 4. engine invariances
def _engine(kind, prob, s, **kw):
    from mv2d_amd.engine import HeadEngine
    return HeadEngine(synthetic.make_head_state(seed=0), kind, torch.device(DEV), num_views=prob['views_per_frame'], roi_size=s, **kw)


def _inputs(prob):
    return torch.from_numpy(prob['feat']).to(DEV), [torch.from_numpy(p) for p in prob['proposals']], prob['img_metas']


def _same(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize('name', ['cfg1_s', 'cfg1_t'])
def test_engine_roi_size_5_invariances(name):
    probs = [synthetic.make_problem(name, seed=s) for s in (0, 3)]
    kind = probs[0]['kind']
    eng = _engine(kind, probs[0], 5)
    ins = [_inputs(p) for p in probs]
    singles = []
    for f, pr, m in ins:
        o = eng.run(f, pr, m)
        assert o['ws']['roi_feat'].shape[1] == 25
        singles.append([t.clone() for t in eng.results(o)])
        assert len(singles[-1][2]) > 0 and bool(torch.isfinite(singles[-1][1]).all())
    if kind == 'S':                                          # the key lists hold 25 cells per listed RoI
        ws, R = o['ws'], o['R']
        rp = ws['row_ptr'][:R + 1].cpu().numpy()
        assert bool((np.diff(rp) % 25 == 0).all()) and bool((np.diff(rp) >= 25).all())
    # several samples through one sequence of launches == each sample alone
    ob = eng.run_batch([f for f, _, _ in ins], [pr for _, pr, _ in ins], [m for _, _, m in ins])
    for b in range(2):
        n = int(ob['count'][b])
        assert n == len(singles[b][2])
        _same((ob['boxes'][b, :n], ob['scores'][b, :n], ob['labels'][b, :n]), singles[b])
    # a graph-replayed frame == an eager one
    f, pr, m = ins[1]
    eng.run(f, ins[0][1], ins[0][2], use_graph=True)       # capture (other boxes), then a replay of sample 1's boxes
    og = eng.run(f, pr, m, use_graph=True)
    _same([t.clone() for t in eng.results(og)], singles[1])


@pytest.mark.parametrize('name', ['cfg1_s', 'cfg1_t'])
def test_engine_roi_size_5_key16_and_fp16_lo_rows(name):
    prob = synthetic.make_problem(name, seed=0)
    f, pr, m = _inputs(prob)
    ref = _engine(prob['kind'], prob, 5)
    r_out = ref.run(f, pr, m)
    k16 = _engine(prob['kind'], prob, 5, exact=False)
    ok = k16.run(f, pr, m)
    lo16 = _engine(prob['kind'], prob, 5)
    lo16.lo8_rows = False
    ol = lo16.run(f, pr, m)
    R = r_out['R']
    c = r_out['cls'][:, :R]
    assert bool(torch.isfinite(c).all())
    assert relerr(ol['cls'][:, :R], c) < 3e-6                  # e4m3 and fp16 lo rows: the same fp32-class key / value rows
    assert relerr(ok['cls'][:, :R], c) < 3e-2                  # one fp16 rounding of the key side


@pytest.mark.parametrize('name', ['cfg1_s', 'cfg1_t'])
def test_engine_roi_size_7_explicit_is_default(name):
    from mv2d_amd.engine import HeadEngine
    prob = synthetic.make_problem(name, seed=1)
    f, pr, m = _inputs(prob)
    a = HeadEngine(synthetic.make_head_state(seed=0), prob['kind'], torch.device(DEV), num_views=prob['views_per_frame'])
    b = _engine(prob['kind'], prob, 7)
    oa, ob = a.run(f, pr, m), b.run(f, pr, m)
    assert torch.equal(oa['cls'], ob['cls']) and torch.equal(oa['reg'], ob['reg'])
    _same(a.results(oa), b.results(ob))


@pytest.mark.parametrize('name', ['cfg1_s', 'cfg1_t'])
def test_engine_roi_size_query_generator_matches_torch(name):
    """The query generator's pooled conv output of the index-exact route against torch float64 on the engine's own RoIAlign output, at s = 5
    and 9 (one chunk / two chunks of 64 cells)."""
    from mv2d_amd import ops
    from oracle import mv2d_oracle as O
    prob = synthetic.make_problem(name, seed=2)
    f, pr, m = _inputs(prob)
    sd = synthetic.make_head_state(seed=0)
    wt = torch.from_numpy(sd['query_generator.shared_convs.0.conv.weight'])
    b = torch.from_numpy(sd['query_generator.shared_convs.0.conv.bias'])
    for s in (5, 9):
        eng = _engine(prob['kind'], prob, s)
        eng.fork_qg = False
        eng.stop_before_decoder = True                       # ws['x2'] (the pooled conv output) is a decoder buffer afterwards
        o = eng.run(f, pr, m)
        ws, R = o['ws'], o['R']
        rois = ws['rois'][:R].cpu()
        want_cells = O.roi_align(f.cpu(), rois, out_size=s).permute(0, 2, 3, 1).reshape(R, s * s, 256)
        hi = ws['roi_feat'][:R].float().cpu()
        assert relerr(hi, want_cells) < 1e-3                  # key16 cells of the s x s RoIAlign
        got = ws['x2'][:R]
        if 'conv' in eng.exact_skip:                           # the key16 conv: against float64 on the rounded operands it read
            wr = ops.f32_to_key16(wt.permute(0, 2, 3, 1).reshape(256, 2304).contiguous().to(DEV)).float().cpu()
            want = _conv_pool_ref(hi, wr.reshape(256, 3, 3, 256).permute(0, 3, 1, 2), b, s)
        else:                                                  # the split-precision conv: against float64 on the fp32 cells
            want = _conv_pool_ref(want_cells, wt, b, s)
        assert relerr(got, want) < 1e-5, s


# ---------------------------------------------------------------------------------------------------------- 5. plugin head and training
def _build(kind, s, use_denoise=None, train=False):
    import mv2d_amd
    cfg = configs.roi_head_cfg_s(roi_size=s) if kind == 'S' else configs.roi_head_cfg_t(roi_size=s)
    if use_denoise is not None:
        cfg['use_denoise'] = use_denoise
    head = mv2d_amd.build_head(cfg, train_cfg=configs.TRAIN_CFG_RCNN if train else None, test_cfg=configs.TEST_CFG_RCNN)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_head_state(seed=0).items()}, strict=not train)
    return head.to(DEV)


@pytest.mark.parametrize('kind,name', [('S', 'cfg1_s'), ('T', 'cfg1_t')])
def test_plugin_simple_test_roi_size_5(kind, name):
    head = _build(kind, 5).eval()
    probs = [synthetic.make_problem(name, seed=s) for s in (0, 4)]
    feats = [torch.from_numpy(p['feat']).to(DEV) for p in probs]
    metas = [[dict(m, box_type_3d=None) for m in p['img_metas']] for p in probs]
    props = [[torch.from_numpy(x) for x in p['proposals']] for p in probs]
    singles = [head.simple_test([feats[b]], props[b], metas[b])[0] for b in range(2)]
    eng = _engine(kind, probs[0], 5)
    _same(singles[0], eng.results(eng.run(feats[0], props[0], probs[0]['img_metas'])))
    got = head.simple_test_batch([torch.cat(feats, 0)], props, metas)
    for b in range(2):
        _same(got[b], singles[b])


def _dropout_off(head):
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    return head


@pytest.mark.parametrize('with_dn', [False, True])
def test_forward_train_roi_size_5_routes_agree(with_dn):
    G, seed = 9, 31
    head = _dropout_off(_build('S', 5, use_denoise=with_dn, train=True))
    prob = synthetic.make_problem('cfg1_s', seed=0)
    gtc = synthetic.make_train_gt(G, seed)
    rnd_ = torch.from_numpy(synthetic.make_dn_noise(G * 10, seed)).to(DEV)
    feat = torch.from_numpy(prob['feat']).to(DEV).requires_grad_(True)
    props = [torch.from_numpy(p) for p in prob['proposals']]
    metas = [dict(m, box_type_3d=None) for m in prob['img_metas']]
    gt_list, lab_list = [torch.from_numpy(gtc['gt'])], [torch.from_numpy(gtc['gt_labels'])]
    hl = head._head_loss(torch.device('cuda', torch.cuda.current_device()))
    seen = {}
    orig_assign = hl.assigner.assign

    def record(*a, **k):
        seen['match'] = orig_assign(*a, **k)
        return seen['match']
    hl.assigner.assign = record
    with torch.no_grad():                                    # the fused route: forward only
        losses = head.forward_train([feat], metas, props, None, None, None, None, gt_list, lab_list, None, dn_noise=rnd_, autograd=False)
    hl.assigner.assign = orig_assign
    # the autograd route with the same assignment (a near-tie of the Hungarian matching may flip under the rounding difference of the routes)
    hl.assigner.assign = lambda *a, **k: seen['match']
    try:
        head.zero_grad(set_to_none=True)
        losses_ag = head.forward_train([feat], metas, props, None, None, None, None, gt_list, lab_list, None, dn_noise=rnd_, autograd=True)
    finally:
        hl.assigner.assign = orig_assign
    assert set(losses_ag) == set(losses) and (any('dn_loss' in k for k in losses) == with_dn)
    for k in losses:
        v = float(losses[k])
        assert np.isfinite(v) and abs(float(losses_ag[k].detach()) - v) <= 2e-3 * max(abs(v), 1e-2), (k, float(losses_ag[k]), v)
    sum(losses_ag.values()).backward()
    grads = {n: p.grad for n, p in head.named_parameters() if p.grad is not None}
    # the gradient reaches the query generator's conv (through the s x s im2col) and the feature map (through the s x s RoIAlign backward)
    for n in ('query_generator.shared_convs.0.conv.weight', 'query_generator.shared_convs.0.conv.bias'):
        assert n in grads and float(grads[n].norm()) > 0, n
    for n, g in grads.items():
        assert bool(torch.isfinite(g).all()), n
    assert feat.grad is not None and bool(torch.isfinite(feat.grad).all()) and float(feat.grad.norm()) > 0


# ---------------------------------------------------------------------------------------------------------- 6. engine vs reference goldens
GOLDEN_CASES = [('cfg2_s', 5), ('cfg3_t', 9), ('nc6_s', 14), ('cfg1_s', 1)]
_RN = load_golden('roi_size_refnoise')


@pytest.mark.parametrize('name,s', GOLDEN_CASES)
def test_engine_matches_reference_golden_roi_size(name, s):
    g = load_golden(f'roi_size_{name}_s{s}')
    key = f'{name}_s{s}_s0'
    noise, gap = int(_RN[key + '_pairwise_ranked_diff'].max()), float(_RN[key + '_max_tie_gap'])
    prob = synthetic.make_problem(name, seed=0)
    eng = _engine(prob['kind'], prob, s, exact=True)
    out = eng.run(torch.from_numpy(prob['feat']).to(DEV), [torch.from_numpy(np.asarray(p)) for p in prob['proposals']], prob['img_metas'],
                  keep_stages=True)
    torch.cuda.synchronize()
    R, st = out['R'], out['stages']
    # per-RoI camera: the reference scales the intrinsics by the RoI size (get_box_params)
    assert relerr(st['enc'][:R, 1024:1040], g['intr']) < 1e-6
    assert relerr(st['center'][:R], g['center_pred']) < 1.3e-4 and relerr(st['xyz'][:R], g['xyz']) < 1.3e-4
    if prob['kind'] == 'T':
        # key list + allowed pairs: bit-exact against the reference's boolean masks
        ffr = unpack_bits(g['feat_for_rois'], g['feat_for_rois_shape'])
        roi_mask = ffr.any(0).reshape(-1)
        np.testing.assert_array_equal(st['roi_mask'].cpu().numpy().astype(bool), roi_mask)
        assert int(st['S_dev'].item()) == int(roi_mask.sum())
        allowed = ffr.reshape(R, -1)[:, roi_mask] & ~g['key_padding'][None]
        rp, ci = st['row_ptr'].cpu().numpy(), st['col_idx'].cpu().numpy()
        for r in range(R):
            np.testing.assert_array_equal(np.sort(ci[rp[r]:rp[r + 1]]), np.nonzero(allowed[r])[0])
    else:
        # the keys of every query: the s*s cells of each RoI of the reference's correlation list (bbox_feats[corr])
        rp, ci = st['row_ptr'].cpu().numpy(), st['col_idx'].cpu().numpy()
        for r in range(R):
            ids = g['corr'][r][g['corr_mask'][r]]
            want = np.sort(np.concatenate([np.arange(s * s) + s * s * int(i) for i in ids]))
            np.testing.assert_array_equal(np.sort(ci[rp[r]:rp[r + 1]]), want)
    e_cls = relerr(out['cls'][:, :R].reshape(g['cls'].shape), g['cls'])
    assert e_cls < 3e-6, e_cls
    n = int(out['count'].item())
    labels = out['labels'][:n].cpu().numpy()
    assert n == len(g['labels'])
    flat = out['bbox_index'][:n].cpu().numpy() * 10 + labels
    ref = g['topk_index']
    assert len(ref) == n
    n_idx = int((flat != ref).sum())
    print(f'[roi_size {s}] {name}: {n_idx}/{n} ranked (query, class) indices differ (reference against itself: {noise}), cls rel err {e_cls:.1e}')
    assert n_idx <= noise
    pos = {int(v): j for j, v in enumerate(ref)}
    for i, v in enumerate(flat):
        if int(v) != int(ref[i]):
            j = pos.get(int(v))
            assert j is not None and abs(float(g['topk_scores'][i]) - float(g['topk_scores'][j])) <= 2.5 * gap, (i, int(v))


# ---------------------------------------------------------------------------------------------------------- 7. training vs the reference at s = 5
def _train_vs_reference(name):
    """Both forward_train routes at s = 5 against the reference's own record (tools/gen_golden_roi_size_train.py): the losses of the fused and
    the autograd route, the gradients of every parameter and of the feature map (bounds of test_gpu_train.py's gradient check).  Returns the
    probe projection of the feature-map gradient and its reference value / norm (checked by the callers)."""
    gold = load_golden('roi_size_train_s5')
    prob_name, kind, G, seed = synthetic.FWD_TRAIN_CASES[name]
    prob = synthetic.make_problem(prob_name, seed=0)
    kind = kind[0]
    import mv2d_amd
    cfg = configs.roi_head_cfg_s(roi_size=5) if kind == 'S' else configs.roi_head_cfg_t(roi_size=5)
    if kind == 'T':
        cfg['num_views'] = prob['views_per_frame']
    head = mv2d_amd.build_head(cfg, train_cfg=configs.TRAIN_CFG_RCNN, test_cfg=configs.TEST_CFG_RCNN)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_head_state(seed=0).items()}, strict=False)
    head = _dropout_off(head.to(DEV))
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
    for got in (losses_f, losses):
        assert set(got) == {k[len(name) + 6:] for k in gold if k.startswith(name + '.loss.')}
        for k in got:
            v = float(gold[f'{name}.loss.{k}'])
            assert abs(float(got[k].detach()) - v) <= 2e-3 * max(abs(v), 1e-2), (k, float(got[k].detach()), v)
    sum(losses.values()).backward()
    params = dict(head.named_parameters())
    names = [str(n) for n in gold[name + '.grad_names']]
    assert len(names) == 232
    worst, errs, top = (0.0, None), [], float(gold[name + '.grad_norm'].max())
    for n, norm, proj in zip(names, gold[name + '.grad_norm'], gold[name + '.grad_proj']):
        g = params[n].grad
        assert g is not None, n
        if norm < 1e-5 * top:
            continue
        g = g.double().cpu()
        got_norm = float(g.norm())
        got_proj = float((g.flatten() * torch.from_numpy(synthetic.grad_probe(n, g.numel())).double()).sum())
        e = max(abs(got_norm - norm), abs(got_proj - proj) / 3.0) / norm
        errs.append(e)
        if e > worst[0]:
            worst = (e, n)
    gf = feat.grad.double().cpu()
    fn = float(gold[name + '.dfeat_norm'])
    assert abs(float(gf.norm()) - fn) <= 2e-2 * fn
    assert torch.allclose(gf.flatten(1).norm(dim=1), torch.from_numpy(gold[name + '.dfeat_view_norms']), rtol=3e-2, atol=1e-3 * fn)
    errs.sort()
    assert worst[0] <= 0.15 and errs[len(errs) // 2] <= 1e-2, (worst, errs[len(errs) // 2])
    proj = float((gf.flatten() * torch.from_numpy(synthetic.grad_probe('feat', gf.numel())).double()).sum())
    return proj, float(gold[name + '.dfeat_proj']), fn


@pytest.mark.parametrize('name', ['train_cfg1_s', 'train_cfg1_t'])
def test_forward_train_roi_size_5_matches_reference(name):
    """Losses of both routes, gradients of all 232 parameters, the feature-map gradient's norm and per-view norms; the T case also its probe
    projection (bound of test_gpu_train.py)."""
    proj, want, fn = _train_vs_reference(name)
    if name == 'train_cfg1_t':
        assert abs(proj - want) <= 8e-2 * fn


@pytest.mark.xfail(strict=True, reason='open: at s = 5 the S head\'s feature-map gradient projects 0.15 x its norm away from the reference\'s '
                                       '(0.019 at s = 7 with the same code; norms, per-view norms and all parameter gradients agree)')
def test_forward_train_roi_size_5_s_head_feature_gradient_projection():
    proj, want, fn = _train_vs_reference('train_cfg1_s')
    assert abs(proj - want) <= 8e-2 * fn


# ---------------------------------------------------------------------------------------------------------- 8. plugin QueryGenerator module
@pytest.mark.parametrize('s', [5, 9])
def test_plugin_query_generator_roi_size(s):
    """QueryGenerator.forward at s != 7 (the fused conv + pool kernel on key16 cells): the pooled conv features against float64 torch on the
    rounded operands; the packed weight is cached per parameter version."""
    from mv2d_amd import ops
    head = _build('S', s).eval()
    qg = head.query_generator
    R = 40
    x = rnd((R, 256, s, s), 900 + s).to(DEV)
    conv = qg.shared_convs[0].conv
    seen = {}
    orig = ops.qg_conv_pool

    def spy(*a, **k):
        r = orig(*a, **k)
        seen['pooled'] = a[3].clone()
        return r
    ops.qg_conv_pool = spy
    try:
        K = torch.eye(4, dtype=torch.float64).repeat(R, 1, 1).to(DEV)
        K[:, 0, 0] = K[:, 1, 1] = 800.0
        K[:, 0, 2], K[:, 1, 2] = 700.0, 250.0
        xyz, _ = qg(x, K, torch.eye(4, dtype=torch.float64).repeat(R, 1, 1).to(DEV), dict(intrinsic=torch.randn(R, 16, device=DEV)))
    finally:
        ops.qg_conv_pool = orig
    assert bool(torch.isfinite(xyz).all()) and xyz.shape == (R, 3)
    xcl = ops.f32_to_key16(x.permute(0, 2, 3, 1).reshape(R, s * s, 256).contiguous()).float().cpu()
    wr = ops.f32_to_key16(conv.weight.detach().permute(0, 2, 3, 1).reshape(256, 2304).contiguous()).float().cpu()
    want = _conv_pool_ref(xcl, wr.reshape(256, 3, 3, 256).permute(0, 3, 1, 2), conv.bias.detach().cpu(), s)
    assert relerr(seen['pooled'], want) < 1e-5
    # the packed conv weight is made once per version of the parameter
    packed = qg._b._c['conv_key16'][1]
    qg(x, K, torch.eye(4, dtype=torch.float64).repeat(R, 1, 1).to(DEV), dict(intrinsic=torch.randn(R, 16, device=DEV)))
    assert qg._b._c['conv_key16'][1] is packed
    with torch.no_grad():
        conv.weight.mul_(1.0)
    qg(x, K, torch.eye(4, dtype=torch.float64).repeat(R, 1, 1).to(DEV), dict(intrinsic=torch.randn(R, 16, device=DEV)))
    assert qg._b._c['conv_key16'][1] is not packed
