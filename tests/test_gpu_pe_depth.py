"""PE depth_num 8 .. 80, depth_start and position_range on the GPU: the fused split-precision PE kernel per first-layer length (csrc/pe_x3_kernel.h),
the frustum-row producers with a row pitch, the engine against the reference goldens tests/golden/pe_depth_*.npz (tools/gen_golden_pe_depth.py),
its invariances at 32 bins, the plugin head at the cfg1_t_d40 config and both forward_train routes at 32 bins."""
import numpy as np
import pytest
import torch

from conftest import load_golden, unpack_bits
from mv2d_amd import configs, synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# the bounds of tests/test_gpu_kernels.py::test_pe_fused_x3_kernel (bf16x3: 2^-17 per operand), tests/test_gpu_roi_size.py (class logits of the
# index-exact route) and tests/test_gpu_golden.py (boxes at equal ranks)
TOL_PE, TOL_CLS, TOL_BOX = 2e-5, 3e-6, 5e-3
RANGE_D40 = [-65.0, -65.0, -8.0, 65.0, 65.0, 8.0]


def relerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def rnd(shape, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def _kp(D):
    return 32 * ((3 * D + 31) // 32)


# ---------------------------------------------------------------------------------------------------------- 1. the PE kernel
_PE_OPERANDS = {}


def _pe_operands(D):
    """Weights, biases, table and their fp64 copies for one depth: built once, shared by the cases, never written."""
    if D not in _PE_OPERANDS:
        from mv2d_amd import ops
        W = {k: v.to(DEV) for k, v in dict(w1a=rnd((1024, 3 * D), 193 + D, 0.08 * (192.0 / (3 * D)) ** 0.5), w1b=rnd((256, 1024), 194, 0.04),
                                            wr=rnd((256, 256), 197, 0.07), we=rnd((256, 256), 198, 0.07)).items()}
        bias = {k: rnd((n,), 199 + i).to(DEV) for i, (k, n) in enumerate(dict(b1a=1024, b1b=256, br=256, be=256).items())}
        wx = {k: ops.pack_x3(ops.pad_pe_w1a(v, D) if k == 'w1a' else v) for k, v in W.items()}
        wx.update(bias)
        tab = rnd((41, 256), 231).to(DEV)
        _PE_OPERANDS[D] = (W, bias, wx, tab)
    return _PE_OPERANDS[D]


def _pe_inputs(D, M, gather):
    NP = M + 50 if gather else M
    A = (rnd((M, 3 * D), 190 + D) * 3.0).to(DEV)
    A1 = torch.zeros((M, _kp(D)), device=DEV)
    A1[:, :3 * D] = A
    Xmap = rnd((NP, 256), 192).to(DEV)
    ri = torch.randperm(NP, generator=torch.Generator().manual_seed(6))[:M].to(torch.int32).to(DEV) if gather else None
    return A, A1, Xmap, ri


def pe_fused_x3_no_size(A1, Xmap, wx, tab, period, pe, Xk, Xv, M, ri):
    """mv2d_pe_fused_x3_fmt, the entry of the 64 bins that has no size argument, called through the library itself (ops.pe_fused_x3 calls the
    size-taking entry for every depth): fp32 / fp16 / bf16 map, rows gathered through ri, (hi, lo) row pairs Xk / Xv with key16 or e4m3 lo rows."""
    from mv2d_amd import _lib, ops
    weights = [wx[k][i].data_ptr() if i < 2 else wx['b' + k[1:]].data_ptr() for k in ('w1a', 'w1b', 'wr', 'we') for i in range(3)]
    assert Xk[1].dtype == Xv[1].dtype
    _lib.check(_lib.load().mv2d_pe_fused_x3_fmt(A1.data_ptr(), Xmap.data_ptr(), ri.data_ptr(), None, M, *weights, tab.data_ptr(), period, pe.data_ptr(),
                                                Xk[0].data_ptr(), Xk[1].data_ptr(), Xv[0].data_ptr(), Xv[1].data_ptr(), int(Xk[1].dtype == torch.uint8), 0, None,
                                                ops.map_format(Xmap.dtype), ops._stream()), 'mv2d_pe_fused_x3_fmt')


@pytest.mark.parametrize('M,gather', [(1, False), (70, True), (200, False), (200, True)])
@pytest.mark.parametrize('D', [8, 24, 32, 40, 64, 80])
def test_pe_fused_x3_depth_against_fp64(D, M, gather):
    """mv2d_pe_fused_x3_k at Kp = 32 .. 256 against fp64 on the UNPADDED operands: construction and bound of test_pe_fused_x3_kernel.  gather: rows
    through row_index and a device-side row count below M."""
    from mv2d_amd import ops
    k16 = ops.key16_dtype()
    W, bias, wx, tab = _pe_operands(D)
    A, A1, Xmap, ri = _pe_inputs(D, M, gather)
    Xrows = Xmap[ri.long()] if gather else Xmap
    Mv = M - 13 if gather else M
    md = torch.tensor([Mv], dtype=torch.int32, device=DEV) if gather else None
    d = lambda t: t.double()                                                            # noqa: E731
    p1 = torch.relu(d(A) @ d(W['w1a']).T + d(bias['b1a'])) @ d(W['w1b']).T + d(bias['b1b'])
    gate = torch.sigmoid(torch.relu(d(Xrows) @ d(W['wr']).T + d(bias['br'])) @ d(W['we']).T + d(bias['be']))
    pos = (ri.long() if gather else torch.arange(M, device=DEV)) % 41
    pe_ref = d(tab)[pos] + p1 * gate
    pe = torch.zeros((M, 256), device=DEV)
    ops.pe_fused_x3(A1, Xmap, md, wx, tab, 41, pe=pe, M=M, row_index=ri, Kp=_kp(D))
    e = relerr(pe[:Mv], pe_ref[:Mv])
    print(f'[pe_x3 depth] D {D} M {M} gather {gather}: pe rel err {e:.2e} (bound {TOL_PE:.0e})')
    assert e < TOL_PE
    assert not pe[Mv:].any()
    # key16 lo rows: hi + lo carry the fp32-class rows (bounds of test_pe_fused_x3_kernel)
    pairs = [tuple(torch.zeros((M, 256), device=DEV, dtype=k16) for _ in range(2)) for _ in range(2)]
    pe2 = torch.zeros((M, 256), device=DEV)
    ops.pe_fused_x3(A1, Xmap, md, wx, tab, 41, pe=pe2, Xk=pairs[0], Xv=pairs[1], M=M, row_index=ri, Kp=_kp(D))
    assert torch.equal(pe2, pe)
    tol = 2e-6 if k16 == torch.float16 else 3e-5
    assert relerr(d(pairs[0][0][:Mv]) + d(pairs[0][1][:Mv]), (pe_ref + d(Xrows))[:Mv]) < TOL_PE + tol
    assert relerr(d(pairs[1][0][:Mv]) + d(pairs[1][1][:Mv]), d(Xrows)[:Mv]) < tol
    assert torch.equal(pairs[1][0][:Mv], Xrows[:Mv].to(k16))
    assert not pairs[0][0][Mv:].any() and not pairs[0][1][Mv:].any()
    if k16 == torch.float16:
        # e4m3 lo rows (256 B): the bytes are the encoding of the key16 lo halves (2^-16 of a product: not held to the key16 bound), the hi rows are untouched
        p8 = [(torch.zeros((M, 256), device=DEV, dtype=k16), torch.zeros((M, 256), device=DEV, dtype=torch.uint8)) for _ in range(2)]
        pe8 = torch.zeros((M, 256), device=DEV)
        ops.pe_fused_x3(A1, Xmap, md, wx, tab, 41, pe=pe8, Xk=p8[0], Xv=p8[1], M=M, row_index=ri, Kp=_kp(D))
        assert torch.equal(pe8, pe)
        for a8, b16 in zip(p8, pairs):
            assert torch.equal(a8[0].view(torch.int16), b16[0].view(torch.int16))
            assert torch.equal(a8[1][:Mv], ops.lo8_encode(b16[1][:Mv])) and not a8[1][Mv:].any()
    if D in (24, 40):
        # whatever the pad columns of a [1024, Kp] copy of the weight hold is dropped by the padding helper, not multiplied: NaN there changes nothing
        Wn = torch.full((1024, _kp(D)), float('nan'), device=DEV)
        Wn[:, :3 * D] = W['w1a']
        wn = dict(wx, w1a=ops.pack_x3(ops.pad_pe_w1a(Wn, D)))
        pe_n = torch.zeros((M, 256), device=DEV)
        ops.pe_fused_x3(A1, Xmap, md, wn, tab, 41, pe=pe_n, M=M, row_index=ri, Kp=_kp(D))
        assert torch.equal(pe_n, pe)


@pytest.mark.parametrize('map_dtype', [torch.float32, torch.float16, torch.bfloat16])
def test_pe_fused_x3_depth_64_is_the_shipped_kernel(map_dtype):
    """Kp = 192 through the size-taking entry runs the instance of mv2d_pe_fused_x3(_fmt): equal bits, for every map element type."""
    from mv2d_amd import ops
    k16 = ops.key16_dtype()
    W, bias, wx, tab = _pe_operands(64)
    for M in (1, 70, 200):
        _, A1, Xmap, ri = _pe_inputs(64, M, True)
        Xmap = Xmap.to(map_dtype)
        outs = []
        for sized in (False, True, None):
            pe = torch.zeros((M, 256), device=DEV)
            pairs = [(torch.zeros((M, 256), device=DEV, dtype=k16), torch.zeros((M, 256), device=DEV, dtype=torch.uint8)) for _ in range(2)]
            if sized is False:
                pe_fused_x3_no_size(A1, Xmap, wx, tab, 41, pe, pairs[0], pairs[1], M, ri)
            else:                                       # (Kp stated, and Kp read from A1's columns)
                ops.pe_fused_x3(A1, Xmap, None, wx, tab, 41, pe=pe, Xk=pairs[0], Xv=pairs[1], M=M, row_index=ri, **(dict(Kp=192) if sized else {}))
            outs.append([pe, *pairs[0], *pairs[1]])
        assert float(outs[0][0].abs().sum()) > 0
        for a, b, c in zip(*outs):
            assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize('D', [32, 40])
@pytest.mark.parametrize('map_dtype', [torch.float16, torch.bfloat16])
def test_pe_fused_x3_depth_16bit_maps_are_exact(D, map_dtype):
    """A 16-bit feature map is widened in the kernel: the results are bitwise those of the fp32 call on x.float()."""
    from mv2d_amd import ops
    k16 = ops.key16_dtype()
    W, bias, wx, tab = _pe_operands(D)
    for M in (1, 70, 200):
        _, A1, Xmap, ri = _pe_inputs(D, M, True)
        x16 = Xmap.to(map_dtype)
        outs = []
        for x in (x16, x16.float()):
            pe = torch.zeros((M, 256), device=DEV)
            pairs = [(torch.zeros((M, 256), device=DEV, dtype=k16), torch.zeros((M, 256), device=DEV, dtype=torch.uint8)) for _ in range(2)]
            ops.pe_fused_x3(A1, x, None, wx, tab, 41, pe=pe, Xk=pairs[0], Xv=pairs[1], M=M, row_index=ri, Kp=_kp(D))
            outs.append([pe, *pairs[0], *pairs[1]])
        assert float(outs[0][0].abs().sum()) > 0
        for a, b in zip(*outs):
            assert torch.equal(a, b)


def test_pe_fused_x3_k_refuses_other_sizes():
    from mv2d_amd import _lib, ops
    W, bias, wx, tab = _pe_operands(8)
    for Kp in (0, 24, 48, 288):
        with pytest.raises(_lib.Mv2dHipError):
            ops.pe_fused_x3(torch.zeros((4, Kp), device=DEV), torch.zeros((4, 256), device=DEV), None, dict(wx, w1a=tuple(t.new_zeros(1024 * Kp) for t in wx['w1a'])),
                            tab, 41, pe=torch.zeros((4, 256), device=DEV), Kp=Kp)


# ---------------------------------------------------------------------------------------------------------- 2. frustum rows with a pitch
@pytest.mark.parametrize('D,start,rng', [(8, 1, None), (40, 2.0, RANGE_D40), (80, 1, None)])
def test_pe_frustum_rows_with_pitch(D, start, rng):
    """mv2d_pe_frustum_f32_ld and mv2d_pe_inputs_ld against the oracle's restatement of MU/pe.py:96-131 the way
    test_pe_frustum_rows_fast_equals_reference_order compares them; the pad columns are exactly 0 (the buffers start as NaN) and rows past the
    list stay untouched."""
    from mv2d_amd import calib, ops
    from oracle import mv2d_oracle as O
    rng = list(O.POST_RANGE) if rng is None else rng
    prob = synthetic.make_problem('micro_t', seed=0)
    metas = prob['img_metas']
    feat = torch.from_numpy(prob['feat'])
    V, C, h, w = feat.shape
    P = V * h * w
    Kp = _kp(D)
    ft = calib.frame_tables(metas, h, w, depth_num=D, depth_start=start, position_range=tuple(rng))
    ct = calib.constant_tables()
    g = np.random.Generator(np.random.PCG64(81))
    sel = np.sort(g.choice(P, size=P // 2, replace=False)).astype(np.int32)
    S = len(sel)
    s2pos = torch.from_numpy(sel).to(DEV)
    S_dev = torch.tensor([S], dtype=torch.int32, device=DEV)
    pr = torch.tensor(rng, dtype=torch.float64)
    T = {k: ft[k].to(DEV) for k in ('img2lidar', 'coords_w', 'coords_h', 'coords_d', 'embeds')}
    nan = float('nan')
    fast = torch.full((P, Kp), nan, device=DEV)
    ops.pe_frustum_f32(s2pos, S_dev, P, T['img2lidar'], T['coords_w'], T['coords_h'], T['coords_d'], fast, V, h, w, D, pr, ld=Kp)
    k16 = ops.key16_dtype()
    slow = torch.full((P, Kp), nan, device=DEV)
    a16 = torch.full((P, Kp), nan, dtype=k16, device=DEV)
    ops.pe_inputs(s2pos, S_dev, P, ops.nchw_to_nhwc(feat.to(DEV)), T['img2lidar'], T['coords_w'], T['coords_h'], T['coords_d'], T['embeds'],
                  ct['dim_t'].to(DEV), a16, torch.zeros((P, 384), dtype=k16, device=DEV), torch.zeros((P, 256), dtype=k16, device=DEV), None, V, h, w, D, pr,
                  A_frustum_f32=slow, A_sine_f32=torch.zeros((P, 384), device=DEV), ld=Kp)
    a16_only = torch.full((P, Kp), nan, dtype=k16, device=DEV)                       # the route without exact rows and without sine rows
    ops.pe_inputs(s2pos, S_dev, P, ops.nchw_to_nhwc(feat.to(DEV)), T['img2lidar'], T['coords_w'], T['coords_h'], T['coords_d'], T['embeds'],
                  ct['dim_t'].to(DEV), a16_only, None, torch.zeros((P, 256), dtype=k16, device=DEV), None, V, h, w, D, pr, ld=Kp)
    ref = O.pe_frustum_input(metas, h, w, depth_num=D, depth_start=start, position_range=rng).permute(0, 2, 3, 1).reshape(P, 3 * D)[sel]
    for rows in (fast, slow, a16, a16_only):
        assert bool((rows[:S, 3 * D:] == 0).all())                                    # the pad columns: exactly 0
        assert bool(torch.isnan(rows[S:]).all())                                       # nothing past the list
    for other, label in ((slow[:S, :3 * D].cpu(), 'pe_inputs_ld (exact rows)'), (ref, 'oracle')):
        dlt = (fast[:S, :3 * D].cpu() - other).abs()
        n_diff = int((dlt > 0).sum())
        print(f'[pe_frustum_f32_ld vs {label}] D {D}: {n_diff} of {dlt.numel()} elements differ, max |diff| {float(dlt.max()):.2e}')
        assert n_diff <= max(1, dlt.numel() // 10000)
        assert float((dlt / other.abs().clamp_min(1e-3)).max()) < 3e-7
    # the key16 rows: the fp32 rows rounded once (bound of test_pe_inputs: one key16 ulp, relative to max(|x|, 1))
    ulp = 2.0 ** -10 if k16 == torch.float16 else 2.0 ** -7
    for rows in (a16, a16_only):
        d16 = (rows[:S, :3 * D].float().cpu() - ref).abs()
        assert float((d16 / ref.abs().clamp_min(1.0)).max()) < ulp
    # without padding (ld = 3 D) the pitch-taking entries run the kernels of the entries without a pitch
    if 3 * D == Kp:
        from mv2d_amd import _lib
        plain = torch.full((P, Kp), nan, device=DEV)
        # (mv2d_pe_frustum_f32 through the library itself: ops.pe_frustum_f32 calls the pitch-taking entry, with or without ld)
        _lib.check(_lib.load().mv2d_pe_frustum_f32(s2pos.data_ptr(), S_dev.data_ptr(), P, T['img2lidar'].data_ptr(), T['coords_w'].data_ptr(),
                                                   T['coords_h'].data_ptr(), T['coords_d'].data_ptr(), plain.data_ptr(), V, h, w, D, pr.data_ptr(),
                                                   ops._stream()), 'mv2d_pe_frustum_f32')
        assert torch.equal(plain[:S], fast[:S])
        no_ld = torch.full((P, Kp), nan, device=DEV)
        ops.pe_frustum_f32(s2pos, S_dev, P, T['img2lidar'], T['coords_w'], T['coords_h'], T['coords_d'], no_ld, V, h, w, D, pr)      # ld=None: 3 D
        assert torch.equal(no_ld[:S], fast[:S])


# ---------------------------------------------------------------------------------------------------------- 3. engine vs the reference goldens
GOLDEN_CASES = [('micro_s_d8', 'micro_s'), ('cfg1_s_d32', 'cfg1_s'), ('cfg1_t_d40', 'cfg1_t'), ('cfg3_t_d80', 'cfg3_t')]
_RN = load_golden('pe_depth_refnoise')


def _pe_keys(g):
    return dict(depth_num=int(g['depth_num']), depth_start=float(g['depth_start']), position_range=tuple(float(v) for v in g['position_range']))


def _state(D):
    return synthetic.with_pe_depth_state(synthetic.make_head_state(seed=0), 0, D)


def _engine(prob, depth_num, **kw):
    from mv2d_amd.engine import HeadEngine
    return HeadEngine(_state(depth_num), prob['kind'], torch.device(DEV), num_views=prob['views_per_frame'], depth_num=depth_num, **kw)


def _inputs(prob):
    return torch.from_numpy(prob['feat']).to(DEV), [torch.from_numpy(np.asarray(p)) for p in prob['proposals']], prob['img_metas']


def _same(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _ranks_vs_golden(flat, g, noise, gap):
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


@pytest.mark.parametrize('case,name', GOLDEN_CASES)
def test_engine_matches_reference_golden_pe_depth(case, name):
    """Every stage test_engine_matches_reference_golden_roi_size compares, with its bounds; ranked indices may differ in at most the case's own
    reference count, each across a reference score gap <= 1e-7."""
    g = load_golden('pe_depth_' + case)
    key = case + '_s0'
    noise, gap = int(_RN[key + '_pairwise_ranked_diff'].max()), float(_RN[key + '_max_tie_gap'])
    prob = synthetic.make_problem(name, seed=0)
    eng = _engine(prob, exact=True, **_pe_keys(g))
    out = eng.run(*_inputs(prob), keep_stages=True)
    torch.cuda.synchronize()
    R, st = out['R'], out['stages']
    s = 7
    assert relerr(st['enc'][:R, 1024:1040], g['intr']) < 1e-6
    assert relerr(st['center'][:R], g['center_pred']) < 1.3e-4 and relerr(st['xyz'][:R], g['xyz']) < 1.3e-4
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
    if 'pe_rows' in g:
        # the engine's PE rows (compact, in key-list order: a keep_stages run) at the recorded map positions some RoI lists
        S = int(st['S_dev'].item())
        s2pos = out['ws']['s2pos'][:S].cpu().numpy()
        row_of = {int(p): i for i, p in enumerate(s2pos)}
        hit = [(row_of[int(p)], j) for j, p in enumerate(g['pe_positions']) if int(p) in row_of]
        assert len(hit) >= 8, len(hit)
        got = st['pe'][:S].cpu()[[i for i, _ in hit]]
        e_pe = relerr(got, g['pe_rows'][[j for _, j in hit]])
        print(f'[pe_depth] {case}: pe rows at {len(hit)} recorded positions: rel err {e_pe:.2e} (bound {TOL_PE:.0e})')
        assert e_pe < TOL_PE
    e_cls = relerr(out['cls'][:, :R].reshape(g['cls'].shape), g['cls'])
    n = int(out['count'].item())
    labels = out['labels'][:n].cpu().numpy()
    print(f'[pe_depth] {case}: cls rel err {e_cls:.2e} (bound {TOL_CLS:.0e}), reference against itself: {noise} ranked indices, gap {gap:.1e}')
    assert e_cls < TOL_CLS, e_cls
    assert n == len(g['labels'])
    n_idx = _ranks_vs_golden(out['bbox_index'][:n].cpu().numpy() * 10 + labels, g, noise, gap)
    print(f'[pe_depth] {case}: {n_idx}/{n} ranked (query, class) indices differ')


# ---------------------------------------------------------------------------------------------------------- 4. engine invariances at 32 bins
@pytest.mark.parametrize('name', ['cfg1_s', 'cfg1_t'])
def test_engine_depth_32_invariances(name):
    probs = [synthetic.make_problem(name, seed=s) for s in (0, 3, 5)]
    eng = _engine(probs[0], 32)
    ins = [_inputs(p) for p in probs]
    singles = []
    for f, pr, m in ins:
        o = eng.run(f, pr, m)
        assert o['ws']['xa1'].shape[1] == 96
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
    # an fp16 map == the fp32 map holding the same values
    f16 = ins[0][0].half()
    a = [t.clone() for t in eng.results(eng.run(f16, ins[0][1], ins[0][2]))]
    b = [t.clone() for t in eng.results(eng.run(f16.float(), ins[0][1], ins[0][2]))]
    _same(a, b)
    # one engine serving alternating RoI-count buckets: a frame with a fifth of the boxes, then the full frames again
    few = [p[:max(1, len(p) // 5)] for p in ins[2][1]]
    fresh = _engine(probs[0], 32)
    want_few = [t.clone() for t in fresh.results(fresh.run(ins[2][0], few, ins[2][2]))]
    for _ in range(2):
        _same([t.clone() for t in eng.results(eng.run(ins[2][0], few, ins[2][2]))], want_few)
        _same([t.clone() for t in eng.results(eng.run(*ins[0]))], singles[0])


def test_engine_depth_refusals():
    """The key16 mode's PE kernel and the rows-in-waves shape stay 64-bin kernels: ValueError before any launch."""
    prob = synthetic.make_problem('cfg1_t', seed=0)
    ins = _inputs(prob)
    with pytest.raises(ValueError, match='depth_num = 64 only'):
        _engine(prob, 32, exact=False).run(*ins)
    eng = _engine(prob, 32)
    eng.pe_rows_in_waves = True
    with pytest.raises(ValueError, match='depth_num = 64 only'):
        eng.run(*ins)


# ---------------------------------------------------------------------------------------------------------- 5. plugin head
def _build(kind, pe_keys, num_views, train=False):
    import mv2d_amd
    cfg = configs.roi_head_cfg_s(**pe_keys) if kind == 'S' else configs.roi_head_cfg_t(**pe_keys)
    if kind == 'T':
        cfg['num_views'] = num_views
    head = mv2d_amd.build_head(cfg, train_cfg=configs.TRAIN_CFG_RCNN if train else None, test_cfg=configs.TEST_CFG_RCNN)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in _state(pe_keys['depth_num']).items()}, strict=not train)
    return head.to(DEV)


def test_plugin_simple_test_matches_golden_cfg1_t_d40():
    """simple_test and simple_test_batch at pe = dict(depth_num=40, depth_start=2.0, position_range=[-65 .. 65, -8 .. 8]) with the coder at
    POST_RANGE: heads.py hands the PE's own start and range to the engine."""
    g = load_golden('pe_depth_cfg1_t_d40')
    key = 'cfg1_t_d40_s0'
    noise, gap = int(_RN[key + '_pairwise_ranked_diff'].max()), float(_RN[key + '_max_tie_gap'])
    prob = synthetic.make_problem('cfg1_t', seed=0)
    keys = _pe_keys(g)
    assert keys['depth_num'] == 40 and keys['depth_start'] == 2.0 and list(keys['position_range']) == RANGE_D40
    head = _build('T', keys, prob['views_per_frame']).eval()
    assert list(head.bbox_head.bbox_coder.post_center_range) == configs.POST_RANGE
    feat = torch.from_numpy(prob['feat']).to(DEV)
    metas = [dict(m, box_type_3d=None) for m in prob['img_metas']]
    props = [torch.from_numpy(x) for x in prob['proposals']]
    single = head.simple_test([feat], props, metas)[0]
    eng = head.engine(feat.device, metas)
    assert eng.depth_start == 2.0 and eng.pe_range_h64.tolist() == RANGE_D40 and eng.post_range_h64.tolist() == configs.POST_RANGE
    batch = head.simple_test_batch([torch.cat([feat, feat], 0)], [props, props], [metas, metas])
    for b in range(2):
        _same(batch[b], single)
    boxes, scores, labels = (t.cpu().numpy() for t in single)
    n = len(labels)
    assert n == len(g['labels'])
    # the ranked labels differ only where ranked indices may (ties of the reference's own scores); scores: sigmoid' <= 1 / 4 of the logit bound
    assert int((labels != g['labels']).sum()) <= noise
    assert float(np.abs(scores - g['scores']).max()) <= 0.25 * TOL_CLS * float(np.abs(g['cls']).max())
    same = labels == g['labels']
    assert float(np.abs(boxes - g['boxes'])[same].max() / np.abs(g['boxes']).max()) < TOL_BOX


# ---------------------------------------------------------------------------------------------------------- 6. training at 32 bins
def _dropout_off(head):
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    return head


@pytest.mark.parametrize('name', ['train_micro_t', 'train_micro_s'])
def test_forward_train_depth_32_matches_reference(name):
    """Both forward_train routes at depth_num = 32 against each other (2e-3 * max(|v|, 1e-2)) and against the reference's own record
    (tools/gen_golden_pe_depth_train.py) under the comparison of tests/test_gpu_roi_size.py::_train_vs_reference: the losses of both routes, the
    gradients of every parameter -- position_encoder.0.weight comes back as [1024, 96, 1, 1] -- and of the feature map."""
    gold = load_golden('pe_depth_train_d32')
    prob_name, kind, G, seed = synthetic.FWD_TRAIN_CASES[name]
    prob = synthetic.make_problem(prob_name, seed=0)
    kind = kind[0]
    head = _dropout_off(_build(kind, dict(depth_num=32), prob['views_per_frame'], train=True))
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
    w1a = 'position_encoding.position_encoder.0.weight'
    assert tuple(params[w1a].grad.shape) == (1024, 96, 1, 1)
    names = [str(n) for n in gold[name + '.grad_names']]
    assert w1a in names
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
        if n == w1a:
            print(f'[pe_depth train] {name}: {w1a} grad norm {got_norm:.4e} (reference {norm:.4e}), rel err {e:.2e}')
        errs.append(e)
        if e > worst[0]:
            worst = (e, n)
    gf = feat.grad.double().cpu()
    fn = float(gold[name + '.dfeat_norm'])
    assert abs(float(gf.norm()) - fn) <= 2e-2 * fn
    assert torch.allclose(gf.flatten(1).norm(dim=1), torch.from_numpy(gold[name + '.dfeat_view_norms']), rtol=3e-2, atol=1e-3 * fn)
    errs.sort()
    assert worst[0] <= 0.15 and errs[len(errs) // 2] <= 1e-2, (worst, errs[len(errs) // 2])
