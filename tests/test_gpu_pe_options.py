"""The PE's with_fpe / no_sin_enc / adapt_pos3d / LID keys on the GPU: the gate-less instance of the fused split-precision PE kernel
(pe_x3_nogate_kernel, mv2d_pe_fused_x3_ng) against fp64 and bit for bit against the shipped kernel with its gate forced to 1, both kernels on a
zero table, the engine against the reference goldens tests/golden/pe_options_*.npz (tools/gen_golden_pe_options.py), its invariances, the
untouched shipped route, the refusals, the plugin head and module-level PE, and both forward_train routes."""
import numpy as np
import pytest
import torch

from conftest import load_golden, unpack_bits
from mv2d_amd import configs, synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# the bounds of tests/test_gpu_pe_depth.py: bf16x3 products (2^-17 per operand), class logits of the index-exact route, boxes at equal ranks
TOL_PE, TOL_CLS, TOL_BOX = 2e-5, 3e-6, 5e-3
TOL_PE_BF16_CHAIN = 1e-2            # tests/test_gpu_plugin.py: the module-level PE.forward (whole map, single-precision bf16 tile GEMM chain)


def relerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def rnd(shape, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def _kp(D):
    return 32 * ((3 * D + 31) // 32)


# ---------------------------------------------------------------------------------------------------------- the PE kernel's operands
_PE_OPERANDS = {}


def _pe_operands(D):
    """tests/test_gpu_pe_depth.py::_pe_operands: weights, biases, table for one depth, built once, shared by the cases, never written."""
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


def _ng(wx):
    """the operands the gate-less entry takes: no wr / we / br / be"""
    return {k: wx[k] for k in ('w1a', 'w1b', 'b1a', 'b1b')}


def _pe_inputs(D, M, gather):
    NP = M + 50 if gather else M
    A = (rnd((M, 3 * D), 190 + D) * 3.0).to(DEV)
    A1 = torch.zeros((M, _kp(D)), device=DEV)
    A1[:, :3 * D] = A
    Xmap = rnd((NP, 256), 192).to(DEV)
    ri = torch.randperm(NP, generator=torch.Generator().manual_seed(6))[:M].to(torch.int32).to(DEV) if gather else None
    return A, A1, Xmap, ri


def _p1_ref(D, A):
    W, bias, _, _ = _pe_operands(D)
    d = lambda t: t.double()                                                            # noqa: E731
    return torch.relu(d(A) @ d(W['w1a']).T + d(bias['b1a'])) @ d(W['w1b']).T + d(bias['b1b'])


def _outs(M, k16, lo8):
    pe = torch.zeros((M, 256), device=DEV)
    pairs = [(torch.zeros((M, 256), device=DEV, dtype=k16), torch.zeros((M, 256), device=DEV, dtype=torch.uint8 if lo8 else k16)) for _ in range(2)]
    return pe, pairs


# ---------------------------------------------------------------------------------------------------------- 1. gate-less kernel vs fp64
@pytest.mark.parametrize('M,gather', [(1, False), (70, True), (200, False), (200, True)])
@pytest.mark.parametrize('D', [8, 40, 64, 80])
def test_pe_fused_x3_nogate_against_fp64(D, M, gather):
    """mv2d_pe_fused_x3_ng at KS1 = 1, 4 (8 pad columns), 6, 8: pe = tab[pos] + relu(A W1a^T + b1a) W1b^T + b1b against fp64 on the unpadded
    operands.  gather: rows through row_index and a device-side row count M - 13."""
    from mv2d_amd import ops
    k16 = ops.key16_dtype()
    W, bias, wx, tab = _pe_operands(D)
    wn = _ng(wx)
    A, A1, Xmap, ri = _pe_inputs(D, M, gather)
    Xrows = Xmap[ri.long()] if gather else Xmap
    Mv = M - 13 if gather else M
    md = torch.tensor([Mv], dtype=torch.int32, device=DEV) if gather else None
    d = lambda t: t.double()                                                            # noqa: E731
    pos = (ri.long() if gather else torch.arange(M, device=DEV)) % 41
    pe_ref = d(tab)[pos] + _p1_ref(D, A)
    pe = torch.zeros((M, 256), device=DEV)
    ops.pe_fused_x3(A1, Xmap, md, wn, tab, 41, pe=pe, M=M, row_index=ri, Kp=_kp(D), gate=False)
    e = relerr(pe[:Mv], pe_ref[:Mv])
    print(f'[pe_x3 nogate] D {D} M {M} gather {gather}: pe rel err {e:.2e} (bound {TOL_PE:.0e})')
    assert e < TOL_PE
    assert not pe[Mv:].any()                                                            # rows at and beyond the device count stay zero
    # a pe-only call without a map: the feature rows are not read
    pe_nomap = torch.zeros((M, 256), device=DEV)
    ops.pe_fused_x3(A1, None, md, wn, tab, 41, pe=pe_nomap, M=M, row_index=ri, Kp=_kp(D), gate=False)
    assert torch.equal(pe_nomap, pe)
    # key16 lo rows: hi + lo carry the fp32-class rows (bounds of test_pe_fused_x3_depth_against_fp64)
    pe2, pairs = _outs(M, k16, False)
    ops.pe_fused_x3(A1, Xmap, md, wn, tab, 41, pe=pe2, Xk=pairs[0], Xv=pairs[1], M=M, row_index=ri, Kp=_kp(D), gate=False)
    assert torch.equal(pe2, pe)
    tol = 2e-6 if k16 == torch.float16 else 3e-5
    assert relerr(d(pairs[0][0][:Mv]) + d(pairs[0][1][:Mv]), (pe_ref + d(Xrows))[:Mv]) < TOL_PE + tol
    assert relerr(d(pairs[1][0][:Mv]) + d(pairs[1][1][:Mv]), d(Xrows)[:Mv]) < tol
    assert torch.equal(pairs[1][0][:Mv], Xrows[:Mv].to(k16))
    for t in (*pairs[0], *pairs[1]):
        assert not t[Mv:].any()
    # the row outputs alone (T path: nothing reads pe)
    _, only = _outs(M, k16, False)
    ops.pe_fused_x3(A1, Xmap, md, wn, tab, 41, Xk=only[0], Xv=only[1], M=M, row_index=ri, Kp=_kp(D), gate=False)
    for a, b in zip((*only[0], *only[1]), (*pairs[0], *pairs[1])):
        assert torch.equal(a, b)
    if k16 == torch.float16:
        # e4m3 lo rows (256 B): the bytes are the encoding of the key16 lo halves, the hi rows are untouched
        pe8, p8 = _outs(M, k16, True)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.pe_fused_x3(A1, Xmap, md, wn, tab, 41, pe=pe8, Xk=p8[0], Xv=p8[1], M=M, row_index=ri, Kp=_kp(D), gate=False, lo8_flag=flag)
        assert torch.equal(pe8, pe) and int(flag.item()) == 0
        for a8, b16 in zip(p8, pairs):
            assert torch.equal(a8[0].view(torch.int16), b16[0].view(torch.int16))
            assert torch.equal(a8[1][:Mv], ops.lo8_encode(b16[1][:Mv])) and not a8[1][Mv:].any()
    if gather:
        # pe_at_index: pe row m is written at row row_index[m] of a position-indexed map
        NP = Xmap.shape[0]
        pe_pos = torch.zeros((NP, 256), device=DEV)
        ops.pe_fused_x3(A1, Xmap, md, wn, tab, 41, pe=pe_pos, M=M, row_index=ri, Kp=_kp(D), gate=False, pe_at_index=True)
        assert torch.equal(pe_pos[ri[:Mv].long()], pe[:Mv])
        rest = torch.ones(NP, dtype=torch.bool, device=DEV)
        rest[ri[:Mv].long()] = False
        assert not pe_pos[rest].any()


# ---------------------------------------------------------------------------------------------------------- 2. the shipped kernel's P1 bits
@pytest.mark.parametrize('D', [8, 64, 80])
def test_pe_fused_x3_nogate_has_the_shipped_p1_bits(D):
    """The gated entry with We = 0 and be = 100 has a gate of exactly 1.0f (1 / (1 + expf(-100)) in fp32) whatever Wr is: its pe, Xk and Xv are the
    gate-less entry's bit for bit -- parts 0..3 of the schedule are the shipped ones."""
    from mv2d_amd import ops
    k16 = ops.key16_dtype()
    W, bias, wx, tab = _pe_operands(D)
    one = dict(wx, we=ops.pack_x3(torch.zeros((256, 256), device=DEV)), be=torch.full((256,), 100.0, device=DEV))
    for M in (1, 70, 200):
        _, A1, Xmap, ri = _pe_inputs(D, M, True)
        outs = []
        for w_, kw in ((one, {}), (_ng(wx), dict(gate=False))):
            pe, pairs = _outs(M, k16, k16 == torch.float16)
            ops.pe_fused_x3(A1, Xmap, None, w_, tab, 41, pe=pe, Xk=pairs[0], Xv=pairs[1], M=M, row_index=ri, Kp=_kp(D), **kw)
            outs.append([pe, *pairs[0], *pairs[1]])
        assert float(outs[0][0].abs().sum()) > 0
        for a, b in zip(*outs):
            assert torch.equal(a, b)
    if D == 64:                                     # ... and through the shipped entry without a size argument (pe_x3_kernel<MT> itself)
        from test_gpu_pe_depth import pe_fused_x3_no_size
        pe, pairs = _outs(M, k16, k16 == torch.float16)
        pe_fused_x3_no_size(A1, Xmap, one, tab, 41, pe, pairs[0], pairs[1], M, ri)
        for a, b in zip([pe, *pairs[0], *pairs[1]], outs[1]):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------- 3. 16-bit maps
@pytest.mark.parametrize('D', [32, 64])
@pytest.mark.parametrize('map_dtype', [torch.float16, torch.bfloat16])
def test_pe_fused_x3_nogate_16bit_maps_are_exact(D, map_dtype):
    """A 16-bit feature map is widened in the kernel: the results are bitwise those of the fp32 call on x.float()."""
    from mv2d_amd import ops
    k16 = ops.key16_dtype()
    W, bias, wx, tab = _pe_operands(D)
    M = 70
    _, A1, Xmap, ri = _pe_inputs(D, M, True)
    md = torch.tensor([M - 13], dtype=torch.int32, device=DEV)
    x16 = Xmap.to(map_dtype)
    outs = []
    for x in (x16, x16.float()):
        pe, pairs = _outs(M, k16, k16 == torch.float16)
        ops.pe_fused_x3(A1, x, md, _ng(wx), tab, 41, pe=pe, Xk=pairs[0], Xv=pairs[1], M=M, row_index=ri, Kp=_kp(D), gate=False)
        outs.append([pe, *pairs[0], *pairs[1]])
    assert float(outs[0][0].abs().sum()) > 0 and float(outs[0][3].float().abs().sum()) > 0
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------- 4. argument errors
def test_pe_fused_x3_ng_argument_errors():
    from mv2d_amd import _lib, ops
    k16 = ops.key16_dtype()
    W, bias, wx, tab = _pe_operands(8)
    wn = _ng(wx)
    for Kp in (0, 48, 288):
        with pytest.raises(_lib.Mv2dHipError, match='Kp'):
            ops.pe_fused_x3(torch.zeros((4, Kp), device=DEV), torch.zeros((4, 256), device=DEV), None, dict(wn, w1a=tuple(t.new_zeros(1024 * Kp) for t in wn['w1a'])),
                            tab, 41, pe=torch.zeros((4, 256), device=DEV), Kp=Kp, gate=False)
    _, A1, Xmap, _ = _pe_inputs(8, 4, False)
    _, pairs = _outs(4, k16, False)
    with pytest.raises(_lib.Mv2dHipError, match='need the feature map'):              # row outputs without a map
        ops.pe_fused_x3(A1, None, None, wn, tab, 41, Xk=pairs[0], Xv=pairs[1], Kp=32, gate=False)
    lib, p = _lib.load(), lambda t: t.data_ptr()
    hi, lo = pairs[0]

    def call(xk_hi, xk_lo, xv_hi, xv_lo):
        return lib.mv2d_pe_fused_x3_ng(p(A1), p(Xmap), None, None, 4, p(wn['w1a'][0]), p(wn['w1a'][1]), p(wn['b1a']), p(wn['w1b'][0]), p(wn['w1b'][1]), p(wn['b1b']),
                                       p(tab), 41, None, xk_hi, xk_lo, xv_hi, xv_lo, 0, 0, None, 0, 32, None)
    for some in ((p(hi), None, None, None), (p(hi), p(lo), None, None), (p(hi), p(lo), p(pairs[1][0]), None), (p(hi), None, p(pairs[1][0]), p(pairs[1][1]))):
        assert call(*some) == -1 and b'come together' in lib.mv2d_last_error()          # only some of the four row outputs
    assert call(None, None, None, None) == -1 and b'no output' in lib.mv2d_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------- 5. a zero table
def test_both_kernels_on_a_one_row_zero_table():
    """no_sin_enc=True: one all-zero table row with tab_period = 1 -- the gated and the gate-less entry equal their fp64 references without a table term."""
    from mv2d_amd import ops
    D, M = 64, 70
    W, bias, wx, _ = _pe_operands(D)
    A, A1, Xmap, ri = _pe_inputs(D, M, True)
    Xrows = Xmap[ri.long()]
    d = lambda t: t.double()                                                            # noqa: E731
    zero = torch.zeros((1, 256), device=DEV)
    p1 = _p1_ref(D, A)
    gate = torch.sigmoid(torch.relu(d(Xrows) @ d(W['wr']).T + d(bias['br'])) @ d(W['we']).T + d(bias['be']))
    for label, w_, kw, ref in (('gated', wx, {}, p1 * gate), ('gate-less', _ng(wx), dict(gate=False), p1)):
        pe = torch.zeros((M, 256), device=DEV)
        ops.pe_fused_x3(A1, Xmap, None, w_, zero, 1, pe=pe, M=M, row_index=ri, **kw)
        e = relerr(pe, ref)
        print(f'[pe_x3 zero table] {label}: pe rel err {e:.2e} (bound {TOL_PE:.0e})')
        assert e < TOL_PE


# ---------------------------------------------------------------------------------------------------------- 6. engine vs the reference goldens
GOLDEN_CASES = [('micro_s_nofpe', 'micro_s'), ('cfg1_t_nofpe', 'cfg1_t'), ('cfg1_s_nosin_uni', 'cfg1_s'), ('micro_t_plain_d40', 'micro_t')]
_RN = load_golden('pe_options_refnoise')
OPT_KEYS = ('with_fpe', 'no_sin_enc', 'adapt_pos3d', 'LID')


def _pe_keys(g):
    return dict(depth_num=int(g['depth_num']), **{k: bool(g[k]) for k in OPT_KEYS})


def _state(keys):
    sd = synthetic.make_head_state(seed=0)
    if keys.get('depth_num', 64) != 64:
        sd = synthetic.with_pe_depth_state(sd, 0, keys['depth_num'])
    return synthetic.with_pe_options_state(sd, keys.get('with_fpe', True), keys.get('no_sin_enc', False))


def _engine(prob, keys, **kw):
    from mv2d_amd.engine import HeadEngine
    return HeadEngine(_state(keys), prob['kind'], torch.device(DEV), num_views=prob['views_per_frame'], **keys, **kw)


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
            assert j is not None and abs(float(g['topk_scores'][i]) - float(g['topk_scores'][j])) <= gap, (i, int(v))
    return n_idx


@pytest.mark.parametrize('case,name', GOLDEN_CASES)
def test_engine_matches_reference_golden_pe_options(case, name):
    """Every stage test_engine_matches_reference_golden_pe_depth compares, with its bounds; pe rows of the micro cases within TOL_PE; ranked indices
    may differ in at most the case's own reference count, each across a reference score gap within the recorded tie gap."""
    g = load_golden('pe_options_' + case)
    seed = int(g['seed'])
    key = f'{case}_s{seed}'
    noise, gap = int(_RN[key + '_pairwise_ranked_diff'].max()), float(_RN[key + '_max_tie_gap'])
    prob = synthetic.make_problem(name, seed=seed)
    keys = _pe_keys(g)
    eng = _engine(prob, keys, exact=True)
    out = eng.run(*_inputs(prob), keep_stages=True)
    torch.cuda.synchronize()
    ws = out['ws']
    assert ('pe_pack' in eng.w) == keys['with_fpe'] and ('wr' in eng.w['pe_x3']) == keys['with_fpe']           # nothing packed for a submodule that is not there
    assert ('pe_w2a_x3' in eng.w) == (not keys['no_sin_enc'])
    if keys['no_sin_enc']:
        assert ws['A2'] is None and ws['xa2'] is None and tuple(ws['shared']['sine_tab'].shape) == (1, 256) and ws['shared']['sine_period'] == 1
        assert not ws['shared']['sine_tab'].any()
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
    assert ('pe_rows' in g) == name.startswith('micro')
    if 'pe_rows' in g:
        # the engine's PE rows (compact, in key-list order: a keep_stages run) at the recorded map positions some RoI lists
        S = int(st['S_dev'].item())
        s2pos = ws['s2pos'][:S].cpu().numpy()
        row_of = {int(p): i for i, p in enumerate(s2pos)}
        hit = [(row_of[int(p)], j) for j, p in enumerate(g['pe_positions']) if int(p) in row_of]
        assert len(hit) >= 8, len(hit)
        got = st['pe'][:S].cpu()[[i for i, _ in hit]]
        e_pe = relerr(got, g['pe_rows'][[j for _, j in hit]])
        print(f'[pe_options] {case}: pe rows at {len(hit)} recorded positions: rel err {e_pe:.2e} (bound {TOL_PE:.0e})')
        assert e_pe < TOL_PE
    e_cls = relerr(out['cls'][:, :R].reshape(g['cls'].shape), g['cls'])
    n = int(out['count'].item())
    labels = out['labels'][:n].cpu().numpy()
    print(f'[pe_options] {case}: cls rel err {e_cls:.2e} (bound {TOL_CLS:.0e}), reference against itself: {noise} ranked indices, gap {gap:.1e}')
    assert e_cls < TOL_CLS, e_cls
    assert n == len(g['labels'])
    n_idx = _ranks_vs_golden(out['bbox_index'][:n].cpu().numpy() * 10 + labels, g, noise, gap)
    print(f'[pe_options] {case}: {n_idx}/{n} ranked (query, class) indices differ')
    same = labels == g['labels']
    assert float(np.abs(out['boxes'][:n].cpu().numpy() - g['boxes'])[same].max() / np.abs(g['boxes']).max()) < TOL_BOX


# ---------------------------------------------------------------------------------------------------------- 7. engine invariances
@pytest.mark.parametrize('name,keys', [('cfg1_t', dict(with_fpe=False)), ('cfg1_s', dict(no_sin_enc=True))], ids=['cfg1_t-nofpe', 'cfg1_s-nosin'])
def test_engine_pe_options_invariances(name, keys):
    probs = [synthetic.make_problem(name, seed=s) for s in (0, 3)]
    eng = _engine(probs[0], keys)
    ins = [_inputs(p) for p in probs]
    singles = []
    for f, pr, m in ins:
        o = eng.run(f, pr, m)
        singles.append([t.clone() for t in eng.results(o)])
        assert len(singles[-1][2]) > 0 and bool(torch.isfinite(singles[-1][1]).all())
    v0 = eng._weights_version
    # two samples through one sequence of launches == each sample alone
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
    # fp16 / bf16 maps == the fp32 map holding the same values
    for dt in (torch.float16, torch.bfloat16):
        f16 = ins[0][0].to(dt)
        a = [t.clone() for t in eng.results(eng.run(f16, ins[0][1], ins[0][2]))]
        b = [t.clone() for t in eng.results(eng.run(f16.float(), ins[0][1], ins[0][2]))]
        _same(a, b)
    # a load_state() bumps the weights version whatever the switches are, and the reloaded engine computes the same
    eng.load_state(_state(keys))
    assert eng._weights_version == v0 + 1
    _same([t.clone() for t in eng.results(eng.run(*ins[0]))], singles[0])


# ---------------------------------------------------------------------------------------------------------- 8. the shipped route
@pytest.mark.parametrize('name', ['cfg1_s', 'cfg1_t'])
def test_engine_defaults_spelled_out_are_the_shipped_route(name):
    """with_fpe=True, no_sin_enc=False, adapt_pos3d=True, LID=True is what an engine built without them runs: equal bits, equal buffers."""
    from mv2d_amd.engine import HeadEngine
    prob = synthetic.make_problem(name, seed=0)
    sd = synthetic.make_head_state(seed=0)
    mk = lambda **kw: HeadEngine(sd, prob['kind'], torch.device(DEV), num_views=prob['views_per_frame'], **kw)      # noqa: E731
    a, b = mk(), mk(with_fpe=True, no_sin_enc=False, adapt_pos3d=True, LID=True)
    assert set(a.w) == set(b.w) and set(a.w['pe_x3']) == set(b.w['pe_x3'])
    oa, ob = a.run(*_inputs(prob), keep_stages=True), b.run(*_inputs(prob), keep_stages=True)
    torch.cuda.synchronize()
    assert {k for k, v in oa['ws'].items() if v is not None} == {k for k, v in ob['ws'].items() if v is not None}
    for k in ('cls', 'reg', 'boxes', 'scores', 'labels', 'bbox_index', 'count'):
        assert torch.equal(oa[k], ob[k]), k
    S = int(oa['stages']['S_dev'].item())
    assert S == int(ob['stages']['S_dev'].item()) and torch.equal(oa['stages']['pe'][:S], ob['stages']['pe'][:S])
    assert torch.equal(oa['ws']['shared']['sine_tab'], ob['ws']['shared']['sine_tab'])


# ---------------------------------------------------------------------------------------------------------- 9. refusals
def test_engine_pe_options_refusals():
    """The key16 mode's PE kernel and the rows-in-waves shape are built for the shipped PE: ValueError naming the key before any launch; a state dict
    laid out for other switches raises naming the switch."""
    from mv2d_amd.engine import HeadEngine
    prob = synthetic.make_problem('cfg1_t', seed=0)
    ins = _inputs(prob)
    keys = dict(with_fpe=False)
    with pytest.raises(ValueError, match='pe_tab96.*with_fpe=True only'):
        _engine(prob, keys, exact=False).run(*ins)
    eng = _engine(prob, keys)
    eng.pe_rows_in_waves = True
    with pytest.raises(ValueError, match='pe_rows_in_waves.*with_fpe=True only'):
        eng.run(*ins)
    eng.pe_rows_in_waves = False
    assert int(eng.run(*ins)['count'].item()) > 0
    full = synthetic.make_head_state(seed=0)
    mk = lambda sd, **kw: HeadEngine(sd, 'T', torch.device(DEV), num_views=prob['views_per_frame'], **kw)        # noqa: E731
    with pytest.raises(ValueError, match='with_fpe=False'):
        mk(full, with_fpe=False)
    with pytest.raises(ValueError, match='with_fpe=True'):
        mk(_state(keys))
    with pytest.raises(ValueError, match='no_sin_enc=True'):
        mk(full, no_sin_enc=True)
    with pytest.raises(ValueError, match='no_sin_enc=False'):
        mk(_state(dict(no_sin_enc=True)))
    with pytest.raises(ValueError, match='with_fpe=False'):
        eng.load_state(full)


# ---------------------------------------------------------------------------------------------------------- 10. plugin
def _build(kind, pe_keys, num_views, train=False):
    import mv2d_amd
    cfg = configs.roi_head_cfg_s(**pe_keys) if kind == 'S' else configs.roi_head_cfg_t(**pe_keys)
    if kind == 'T':
        cfg['num_views'] = num_views
    head = mv2d_amd.build_head(cfg, train_cfg=configs.TRAIN_CFG_RCNN if train else None, test_cfg=configs.TEST_CFG_RCNN)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in _state(pe_keys).items()}, strict=not train)
    return head.to(DEV)


def test_plugin_simple_test_matches_golden_cfg1_t_nofpe():
    """simple_test and simple_test_batch of an MV2DTHead built from roi_head_cfg_t(with_fpe=False): heads.py hands the PE's switches to the engine."""
    g = load_golden('pe_options_cfg1_t_nofpe')
    seed = int(g['seed'])
    key = f'cfg1_t_nofpe_s{seed}'
    noise = int(_RN[key + '_pairwise_ranked_diff'].max())
    prob = synthetic.make_problem('cfg1_t', seed=seed)
    head = _build('T', dict(with_fpe=False), prob['views_per_frame']).eval()
    assert not hasattr(head.position_encoding, 'fpe')
    feat = torch.from_numpy(prob['feat']).to(DEV)
    metas = [dict(m, box_type_3d=None) for m in prob['img_metas']]
    props = [torch.from_numpy(x) for x in prob['proposals']]
    single = head.simple_test([feat], props, metas)[0]
    eng = head.engine(feat.device, metas)
    assert eng.with_fpe is False and eng.no_sin_enc is False and eng.LID is True
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


def test_plugin_module_level_pe_forward_plain_d40():
    """PE.forward (the whole map through the bf16 tile GEMM chain) with every switch off at 40 bins against the reference's pe rows."""
    g = load_golden('pe_options_micro_t_plain_d40')
    keys = _pe_keys(g)
    assert keys == dict(depth_num=40, with_fpe=False, no_sin_enc=True, adapt_pos3d=False, LID=False)
    prob = synthetic.make_problem('micro_t', seed=int(g['seed']))
    head = _build('T', keys, prob['views_per_frame']).eval()
    pe_mod = head.position_encoding
    assert sorted(n for n, _ in pe_mod.named_children()) == ['position_encoder']
    feat = torch.from_numpy(prob['feat']).to(DEV)
    pe = pe_mod([feat], prob['img_metas'])[0]
    V, C, h, w = pe.shape
    rows = pe.permute(0, 2, 3, 1).reshape(V * h * w, C)[torch.from_numpy(g['pe_positions']).long().to(DEV)]
    e = relerr(rows, g['pe_rows'])
    print(f'[pe_options] module-level PE.forward, micro_t_plain_d40: rel err {e:.2e} (bound {TOL_PE_BF16_CHAIN:.0e})')
    assert e < TOL_PE_BF16_CHAIN


# ---------------------------------------------------------------------------------------------------------- 11. training
def _dropout_off(head):
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    return head


@pytest.mark.parametrize('name,keys', [('train_micro_t', dict(with_fpe=False)), ('train_micro_s', dict(no_sin_enc=True, LID=False))],
                         ids=['train_micro_t-nofpe', 'train_micro_s-nosin_uni'])
def test_forward_train_pe_options_matches_reference(name, keys):
    """Both forward_train routes against each other (2e-3 * max(|v|, 1e-2)) and against the reference's own record
    (tools/gen_golden_pe_options_train.py) under the comparison of test_forward_train_depth_32_matches_reference: the losses of both routes, the
    gradients of every parameter the PE still has, and of the feature map."""
    gold = load_golden('pe_options_train')
    prob_name, kind, G, seed = synthetic.FWD_TRAIN_CASES[name]
    prob = synthetic.make_problem(prob_name, seed=0)
    kind = kind[0]
    head = _dropout_off(_build(kind, keys, prob['views_per_frame'], train=True))
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
    assert tuple(params[w1a].grad.shape) == (1024, 192, 1, 1)
    names = [str(n) for n in gold[name + '.grad_names']]
    assert w1a in names and set(names) <= set(params)
    assert not any(('.fpe.' in n and not keys.get('with_fpe', True)) or ('.adapt_pos3d.' in n and keys.get('no_sin_enc', False)) for n in params)
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
            print(f'[pe_options train] {name}: {w1a} grad norm {got_norm:.4e} (reference {norm:.4e}), rel err {e:.2e}')
        errs.append(e)
        if e > worst[0]:
            worst = (e, n)
    gf = feat.grad.double().cpu()
    fn = float(gold[name + '.dfeat_norm'])
    assert abs(float(gf.norm()) - fn) <= 2e-2 * fn
    assert torch.allclose(gf.flatten(1).norm(dim=1), torch.from_numpy(gold[name + '.dfeat_view_norms']), rtol=3e-2, atol=1e-3 * fn)
    errs.sort()
    assert worst[0] <= 0.15 and errs[len(errs) // 2] <= 1e-2, (worst, errs[len(errs) // 2])
