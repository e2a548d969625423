"""fp16 and bf16 feature maps taken natively (-m gpu).  The reference head widens a mixed-precision backbone's map with x.float() (force_fp32),
which is exact, and the kernels here widen each element in registers and then do the fp32 kernels' arithmetic -- so every expected value below
is this library's own fp32 path fed x16.float(), and every comparison is bitwise (torch.equal): the transposition (full, masked, fallback),
RoIAlign in every output form at s = 1, 5, 7, 14, pe_inputs, the PE block on both routes; the engine (S and T: layouts, batches, graph replay,
key16 mode, fp16 lo rows, roi_size 5, 3 classes, the debugging / training options, alternating dtypes on one engine); the plugin head (inference,
both training routes, the dtype of feat.grad); one full-size cfg2_s and cfg3_t sample."""
import numpy as np
import pytest
import torch

from mv2d_amd import configs, synthetic
from test_gpu_roi_size import _rois

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = [torch.float16, torch.bfloat16]
IDS = ['fp16', 'bf16']


def rnd16(shape, seed, dtype, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32)).to(dtype)


def rnd(shape, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def bits(t):
    """Bitwise view for comparisons (NaN-proof, sign-of-zero-proof)."""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------- 1. transposition
# (V, C, h, w): HW % 8 == 0 | HW % 8 == 4 | the 88 x 32 map of the 1408 x 512 configs | C not a multiple of 64 | fallback (HW % 4 != 0) | fallback (C % 4 != 0)
TR_SHAPES = [(2, 256, 8, 16), (3, 256, 3, 4), (2, 256, 32, 88), (2, 100, 6, 10), (2, 256, 3, 5), (1, 6, 4, 4), (2, 256, 5, 13)]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', TR_SHAPES)
def test_transposition_16bit(shape, dtype):
    from mv2d_amd import ops
    V, Cn, h, w = shape
    x = rnd16(shape, 7 + h, dtype, 3.0).to(DEV)
    # includes fp16 subnormals, the largest finite values and signed zeros: the elements are moved, not interpreted
    x.view(-1)[:6] = torch.tensor([6e-8, -6e-8, 65504.0, -65504.0, 0.0, -0.0], dtype=torch.float32).to(dtype).to(DEV)
    got = ops.nchw_to_nhwc(x)
    want = ops.nchw_to_nhwc(x.float()).to(dtype)
    assert got.dtype == dtype and same(got, want)
    assert same(got, x.permute(0, 2, 3, 1).reshape(V * h * w, Cn).contiguous())
    if (h * w) % 4 == 0 and Cn % 4 == 0:
        # masked form: only the listed rows are written, the others keep what they held
        g = torch.Generator().manual_seed(h * w)
        mask = (torch.rand(V * h * w, generator=g) < 0.4).to(torch.uint8)
        mask[:70] = 0                                          # a whole 64-position block without a listed row
        mask = mask.to(DEV)
        old = rnd16((V * h * w, Cn), 99, dtype).to(DEV)
        out16 = old.clone()
        out32 = old.float()
        ops.nchw_to_nhwc(x, out16, mask=mask)
        ops.nchw_to_nhwc(x.float(), out32, mask=mask)
        assert same(out16, out32.to(dtype))
        keep = mask == 0
        assert same(out16[keep], old[keep]) and same(out16[~keep], got[~keep])
        # per-sample list form: slices of one buffer, one call per map
        buf = torch.zeros((V * h * w, Cn), dtype=dtype, device=DEV)
        for v in range(V):
            ops.nchw_to_nhwc(x[v:v + 1].contiguous(), buf[v * h * w:(v + 1) * h * w])
        assert same(buf, got)


def test_transposition_rejects_mixed_dtypes():
    from mv2d_amd import _lib, ops
    x = torch.zeros((1, 8, 2, 2), dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.Mv2dHipError):
        ops.nchw_to_nhwc(x, torch.zeros((4, 8), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match='float32.*float16.*bfloat16'):
        ops.nchw_to_nhwc(x.double())


# ---------------------------------------------------------------------------------------------------------- 2. RoIAlign
def _roi_align_forms(ops, m0, comp, index, full1, rois, h, w, s):
    """Every output form of the kernel on the feature map m0 (any dtype): a dict of named output tensors."""
    R, k16 = rois.shape[0], ops.key16_dtype()
    e16 = lambda: torch.zeros((R, s * s, 256), device=DEV, dtype=k16)             # noqa: E731
    e32 = lambda: torch.zeros((R, s * s, 256), device=DEV)                        # noqa: E731
    e8 = lambda: torch.zeros((R, s * s, 256), device=DEV, dtype=torch.uint8)      # noqa: E731
    o = {}
    # key16 + both fp32 outputs, map1 compacted behind an index
    o['a0'], o['a0f'], o['a1f'], o['a1'] = e16(), e32(), e32(), e16()
    ops.roi_align(m0, rois, h, w, map1=comp, map1_index=index, out0=o['a0'], out1=o['a1'], out0_f32=o['a0f'], out1_f32=o['a1f'], R=R, roi_size=s)
    # key16 hi + lo pairs, out1 as the sum (the S path's key rows), position-indexed map1
    o['b0'], o['b0l'], o['b1'], o['b1l'] = e16(), e16(), e16(), e16()
    ops.roi_align(m0, rois, h, w, map1=full1, out0=o['b0'], out1=o['b1'], out1_is_sum=True, out0_lo=o['b0l'], out1_lo=o['b1l'], R=R, roi_size=s)
    # lo8 rows (+ the key16 lo cells of the conv input), the saturation flag
    o['c0'], o['c0l'], o['c08'], o['c1'], o['c18'] = e16(), e16(), e8(), e16(), e8()
    o['cflag'] = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.roi_align(m0, rois, h, w, map1=comp, map1_index=index, out0=o['c0'], out1=o['c1'], out1_is_sum=True, out0_lo=o['c0l'], out0_lo8=o['c08'],
                  out1_lo8=o['c18'], lo8_flag=o['cflag'], R=R, roi_size=s)
    # the feature half alone (T path), key16 and fp32
    o['d0'], o['d0l'], o['d0f'] = e16(), e16(), e32()
    ops.roi_align(m0, rois, h, w, out0=o['d0'], out0_lo=o['d0l'], out0_f32=o['d0f'], R=R, roi_size=s)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('s', [1, 5, 7, 14])
def test_roi_align_16bit_map_every_output_form(s, dtype):
    from mv2d_amd import ops
    V, h, w = 2, 12, 20
    f0 = rnd16((V, 256, h, w), 10 + s, dtype, 2.0)
    f0.view(-1)[:3] = torch.tensor([6e-8, 300.0, -300.0]).to(dtype)               # a subnormal; |x| > 224 (the lo8 saturation flag)
    f1 = rnd((V, 256, h, w), 40 + s)
    rois = _rois(V, h, w, s).to(DEV)
    m16 = f0.permute(0, 2, 3, 1).reshape(-1, 256).contiguous().to(DEV)
    full1 = f1.permute(0, 2, 3, 1).reshape(-1, 256).contiguous()
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(s)).permutation(full1.shape[0]))
    comp = full1[perm].contiguous().to(DEV)
    index = torch.empty(full1.shape[0], dtype=torch.int32)
    index[perm] = torch.arange(full1.shape[0], dtype=torch.int32)
    index, full1 = index.to(DEV), full1.to(DEV)
    got = _roi_align_forms(ops, m16, comp, index, full1, rois, h, w, s)
    want = _roi_align_forms(ops, m16.float(), comp, index, full1, rois, h, w, s)
    for k in want:
        assert same(got[k], want[k]), k
    assert float(want['a0f'].abs().sum()) > 0 and float(want['c18'].float().abs().sum()) > 0


# ---------------------------------------------------------------------------------------------------------- 3. PE kernels
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('exact_rows', [False, True])
def test_pe_inputs_16bit_map(exact_rows, dtype):
    from mv2d_amd import calib, ops
    from oracle import mv2d_oracle as O
    prob = synthetic.make_problem('cfg1_t', seed=0)
    metas = prob['img_metas']
    feat = torch.from_numpy(prob['feat']).to(dtype)
    V, C, h, w = feat.shape
    P = V * h * w
    ft, ct = calib.frame_tables(metas, h, w), calib.constant_tables()
    g = np.random.Generator(np.random.PCG64(80))
    sel = np.sort(g.choice(P, size=P // 3, replace=False)).astype(np.int32)
    s2pos, S_dev = torch.from_numpy(sel).to(DEV), torch.tensor([len(sel)], dtype=torch.int32, device=DEV)
    k16 = ops.key16_dtype()
    tabs = [ft[k].to(DEV) for k in ('img2lidar', 'coords_w', 'coords_h', 'coords_d', 'embeds')] + [ct['dim_t'].to(DEV)]

    def run(fcl):
        o = dict(A1=torch.zeros((P, 192), dtype=k16, device=DEV), A2=torch.zeros((P, 384), dtype=k16, device=DEV),
                 Xb=torch.zeros((P, 256), dtype=k16, device=DEV), Xf=torch.zeros((P, 256), device=DEV))
        if exact_rows:
            o['A1f'], o['A2f'] = torch.zeros((P, 192), device=DEV), torch.zeros((P, 384), device=DEV)
        ops.pe_inputs(s2pos, S_dev, P, fcl, *tabs, o['A1'], o['A2'], o['Xb'], o['Xf'], V, h, w, 64, torch.tensor(O.POST_RANGE, dtype=torch.float64),
                      A_frustum_f32=o.get('A1f'), A_sine_f32=o.get('A2f'))
        # the frustum-only form (A_sine = None: the inference path of the key16 mode)
        o['A1n'], o['Xbn'] = torch.zeros((P, 192), dtype=k16, device=DEV), torch.zeros((P, 256), dtype=k16, device=DEV)
        if not exact_rows:
            ops.pe_inputs(s2pos, S_dev, P, fcl, *tabs, o['A1n'], None, o['Xbn'], None, V, h, w, 64, torch.tensor(O.POST_RANGE, dtype=torch.float64))
        torch.cuda.synchronize()
        return o
    fcl16 = ops.nchw_to_nhwc(feat.to(DEV))
    got, want = run(fcl16), run(fcl16.float())
    for k in want:
        assert same(got[k], want[k]), k
    assert same(got['Xf'][:len(sel)], fcl16[torch.from_numpy(sel).long().to(DEV)].float())


def _pe_weights(ops, seed, pack):
    W = {k: v.to(DEV) for k, v in dict(w1a=rnd((1024, 192), seed + 3, 0.08), w1b=rnd((256, 1024), seed + 4, 0.04), wr=rnd((256, 256), seed + 7, 0.07),
                                        we=rnd((256, 256), seed + 8, 0.07)).items()}
    wx = {k: pack(v) for k, v in W.items()}
    wx.update({k: rnd((n,), seed + 9 + i).to(DEV) for i, (k, n) in enumerate(dict(b1a=1024, b1b=256, br=256, be=256).items())})
    return wx


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('M,use_mdev,use_ri,rows,lo8,at_index', [(63, False, False, False, False, False), (130, False, True, True, False, False),
                                                                 (1000, True, True, True, True, False), (517, False, True, False, False, True),
                                                                 (8794, True, False, True, True, False)])
def test_pe_fused_x3_16bit_map(M, use_mdev, use_ri, rows, lo8, at_index, dtype):
    from mv2d_amd import ops
    k16 = ops.key16_dtype()
    NP = M + 50 if use_ri else M
    A1 = (rnd((M, 192), 190) * 3.0).to(DEV)
    X16 = rnd16((NP, 256), 192, dtype).to(DEV)
    X16.view(-1)[:2] = torch.tensor([6e-8, 250.0]).to(dtype).to(DEV)
    ri = torch.randperm(NP, generator=torch.Generator().manual_seed(6))[:M].to(torch.int32).to(DEV) if use_ri else None
    wx = _pe_weights(ops, 190, ops.pack_x3)
    period = 41
    tab = rnd((period, 256), 231).to(DEV)
    md = torch.tensor([M - 13], dtype=torch.int32, device=DEV) if use_mdev else None

    def run(Xmap):
        pe = torch.zeros((NP if at_index else M, 256), device=DEV)
        hi = lambda: torch.zeros((M, 256), device=DEV, dtype=k16)                                        # noqa: E731
        lo = lambda: torch.zeros((M, 256), device=DEV, dtype=torch.uint8 if lo8 else k16)                # noqa: E731
        pairs = [(hi(), lo()), (hi(), lo())] if rows else [None, None]
        flag = torch.zeros(1, dtype=torch.int32, device=DEV) if lo8 else None
        ops.pe_fused_x3(A1, Xmap, md, wx, tab, period, pe=pe, Xk=pairs[0], Xv=pairs[1], M=M, row_index=ri, pe_at_index=at_index, lo8_flag=flag)
        torch.cuda.synchronize()
        return [pe] + ([t for p in pairs for t in p] if rows else []) + ([flag] if lo8 else [])
    got, want = run(X16), run(X16.float())
    assert len(got) == len(want) and float(want[0].abs().sum()) > 0
    for i, (a, b) in enumerate(zip(got, want)):
        assert same(a, b), i


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('M,use_mdev,use_ri', [(95, False, False), (97, False, True), (1000, True, True), (8794, True, False)])
def test_pe_fused_tab_16bit_map(M, use_mdev, use_ri, dtype):
    from mv2d_amd import ops
    k16 = ops.key16_dtype()
    NP = M + 50 if use_ri else M
    A1 = rnd((M, 192), 90).to(DEV).to(k16)
    X16 = rnd16((NP, 256), 92, dtype).to(DEV)
    ri = torch.randperm(NP, generator=torch.Generator().manual_seed(5))[:M].to(torch.int32).to(DEV) if use_ri else None
    Xfb = (X16[ri.long()] if use_ri else X16).float().to(k16)
    wp = _pe_weights(ops, 90, ops.pack_key16)
    period = 37
    tab = rnd((period, 256), 131).to(DEV)
    md = torch.tensor([M - 13], dtype=torch.int32, device=DEV) if use_mdev else None
    for shape in (1, 0):
        outs = []
        for Xmap in (X16, X16.float()):
            pe, xk = torch.zeros((M, 256), device=DEV), torch.zeros((M, 256), device=DEV, dtype=k16)
            ops.pe_fused_tab(A1, Xfb, Xmap, md, wp, tab, period, pe, xk, M=M, row_index=ri, shape=shape)
            xk_only = torch.zeros((M, 256), device=DEV, dtype=k16)
            ops.pe_fused_tab(A1, Xfb, Xmap, md, wp, tab, period, None, xk_only, M=M, row_index=ri, shape=shape)
            torch.cuda.synchronize()
            outs.append((pe, xk, xk_only))
        for a, b in zip(*outs):
            assert same(a, b), shape
        assert float(outs[0][1].float().abs().sum()) > 0


# ---------------------------------------------------------------------------------------------------------- 4. engine
def _engine(prob, **kw):
    from mv2d_amd.engine import HeadEngine
    nc = kw.get('num_classes', 10)
    return HeadEngine(synthetic.make_head_state(seed=0, num_classes=nc), prob['kind'], torch.device(DEV), num_views=prob['views_per_frame'], **kw)


def _inputs(prob):
    return torch.from_numpy(prob['feat']).to(DEV), [torch.from_numpy(p) for p in prob['proposals']], prob['img_metas']


def _layout(x, layout):
    return x.contiguous(memory_format=torch.channels_last) if layout == 'channels_last' else x.contiguous()


def _snap(eng, out):
    """Everything a caller can read from a frame, copied out of the workspace (the next run on the same bucket rewrites it)."""
    ws, R = out['ws'], out['R']
    torch.cuda.synchronize()
    eng._check_capacity(ws)
    rp = ws['row_ptr'][:R + 1].clone()
    d = dict(cls=out['cls'].clone(), reg=out['reg'].clone(), boxes=out['boxes'].clone(), scores=out['scores'].clone(), labels=out['labels'].clone(),
             bbox_index=out['bbox_index'].clone(), count=out['count'].clone(), row_ptr=rp, col_idx=ws['col_idx'][:int(rp[R])].clone())
    assert int(d['count'].sum()) > 0 and bool(torch.isfinite(d['scores']).all())
    return d


def _assert_same(got, want):
    assert set(got) == set(want)
    for k in want:
        assert same(got[k], want[k]), k


@pytest.mark.parametrize('layout', ['nchw', 'channels_last'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('name', ['cfg1_s', 'cfg1_t'])
def test_engine_16bit_map_equals_upcast_map(name, dtype, layout):
    prob = synthetic.make_problem(name, seed=0)
    f, pr, m = _inputs(prob)
    x16 = _layout(f.to(dtype), layout)
    eng = _engine(prob)
    want = _snap(eng, eng.run(x16.float(), pr, m))
    out = eng.run(x16, pr, m)
    ws = out['ws']
    assert ws['featcl'].dtype == dtype and ws['featcl_cur'].dtype == dtype and ws['map_dtype'] == dtype
    if layout == 'channels_last':                            # zero-copy: the position-major map IS the input's storage
        assert ws['featcl_cur'].data_ptr() == x16.data_ptr() and ws['featcl_cur'].untyped_storage().data_ptr() == x16.untyped_storage().data_ptr()
    _assert_same(_snap(eng, out), want)


VARIANTS = ['batch_stacked', 'batch_list', 'graph', 'key16', 'fp16_lo_rows', 'roi_size_5', 'num_classes_3']


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('name', ['cfg1_s', 'cfg1_t'])
def test_engine_16bit_map_variants(name, variant):
    probs = [synthetic.make_problem(name, seed=s) for s in (0, 3)]
    kw = {'key16': dict(exact=False), 'roi_size_5': dict(roi_size=5), 'num_classes_3': dict(num_classes=3)}.get(variant, {})
    eng = _engine(probs[0], **kw)
    if variant == 'fp16_lo_rows':
        eng.lo8_rows = False
    ins = [_inputs(p) for p in probs]
    for dtype in DTYPES:
        xs = [f.to(dtype) for f, _, _ in ins]
        prs, ms = [pr for _, pr, _ in ins], [m for _, _, m in ins]
        if variant == 'batch_stacked':
            run = lambda up: eng.run_batch(torch.cat([up(x) for x in xs]), prs, ms)                    # noqa: E731
        elif variant == 'batch_list':
            run = lambda up: eng.run_batch([up(x) for x in xs], prs, ms)                               # noqa: E731
        elif variant == 'graph':
            bufs = {}

            def run(up):
                x = bufs.setdefault(up, up(xs[1]))                 # (a static input buffer per dtype: its address is in the graph key)
                n = len(eng.run(x, prs[0], ms[0], use_graph=True)['ws']['graphs'])          # capture with other boxes ...
                first = _snap(eng, eng.run(x, prs[1], ms[1], use_graph=True))
                again = eng.run(x, prs[1], ms[1], use_graph=True)  # ... and replays: no further capture
                _assert_same(_snap(eng, again), first)
                assert len(again['ws']['graphs']) == n
                return again
        else:
            run = lambda up: eng.run(up(xs[1]), prs[1], ms[1])                                         # noqa: E731
        want = _snap(eng, run(lambda x: x.float()))
        out = run(lambda x: x)
        assert out['ws']['featcl'].dtype == dtype
        _assert_same(_snap(eng, out), want)
        if variant == 'graph':                                 # the graph-replayed 16-bit frame == the eager one
            _assert_same(_snap(eng, eng.run(xs[1], prs[1], ms[1])), want)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('name', ['cfg1_s', 'cfg1_t'])
def test_engine_16bit_map_debug_and_training_options(name, dtype):
    """keep_stages, debug_attn, stop_before_decoder, keep_sine_rows, pe_input_rows and train_forward all read the 16-bit position-major map."""
    prob = synthetic.make_problem(name, seed=2)
    f, pr, m = _inputs(prob)
    x16 = f.to(dtype)
    V, _, h, w = f.shape

    def stages(x, **opts):
        eng = _engine(prob)
        for k, v in opts.items():
            setattr(eng, k, v)
        out = eng.run(x, pr, m, keep_stages=True)
        torch.cuda.synchronize()
        st = dict(out['stages'])
        R, ws = out['R'], out['ws']
        S = int(st['S_dev'])
        for k in ('pe', 'Xk', 'Xf_b', 's2pos'):                # rows behind the S listed positions are never written
            if k in st:
                st[k] = st[k][:S]
        st['col_idx'] = st['col_idx'][:int(st['row_ptr'][R])]
        if name == 'cfg1_s':
            st.pop('Xk', None)                                   # (S path, index-exact route: nothing writes Xk ...
            if not opts.get('keep_sine_rows'):
                st.pop('Xf_b', None)                             #  ... and only the training route's pe_inputs writes the key16 feature rows)
        if opts.get('stop_before_decoder'):
            for k in ('outs', 'cls', 'reg'):
                st.pop(k)
        st['A2'] = ws['A2'][:S].clone() if opts.get('keep_sine_rows') else None
        pos = torch.arange(0, V * h * w, 97, dtype=torch.int32, device=DEV)
        st['rows16'], st['rows32'] = eng.pe_input_rows(ws, pos, V, h, w), eng.pe_input_rows(ws, pos, V, h, w, f32=True)
        if not opts.get('stop_before_decoder'):
            st['train'] = eng.train_forward(out)
        return {k: v for k, v in st.items() if v is not None}

    for opts in (dict(), dict(debug_attn=True), dict(keep_sine_rows=True), dict(stop_before_decoder=True, keep_sine_rows=True)):
        got, want = stages(x16, **opts), stages(x16.float(), **opts)
        assert set(got) == set(want)
        for k in want:
            a, b = (got[k], want[k]) if isinstance(want[k], (tuple, list)) else ([got[k]], [want[k]])
            for x, y in zip(a, b):
                assert same(x, y), (opts, k)


@pytest.mark.parametrize('name', ['cfg1_s', 'cfg1_t'])
def test_one_engine_alternating_map_dtypes(name):
    prob = synthetic.make_problem(name, seed=1)
    f, pr, m = _inputs(prob)
    maps = {torch.float32: f, torch.float16: f.to(torch.float16), torch.bfloat16: f.to(torch.bfloat16)}
    ref = _engine(prob)
    want = {dt: _snap(ref, ref.run(x.float(), pr, m)) for dt, x in maps.items()}
    assert not same(want[torch.float32]['cls'], want[torch.float16]['cls']) and not same(want[torch.float16]['cls'], want[torch.bfloat16]['cls'])
    eng = _engine(prob)
    order = [torch.float32, torch.float16, torch.bfloat16, torch.float32, torch.bfloat16, torch.float16]
    for use_graph in (False, True, True):
        for dt in order:
            out = eng.run(maps[dt], pr, m, use_graph=use_graph)
            assert out['ws']['featcl'].dtype == dt
            _assert_same(_snap(eng, out), want[dt])
    assert len({id(w) for w in eng._ws.values()}) == 3


def test_engine_refuses_mixed_and_unsupported_dtypes():
    probs = [synthetic.make_problem('cfg1_s', seed=s) for s in (0, 3)]
    ins = [_inputs(p) for p in probs]
    eng = _engine(probs[0])
    prs, ms = [pr for _, pr, _ in ins], [m for _, _, m in ins]
    with pytest.raises(ValueError, match='one dtype'):
        eng.run_batch([ins[0][0].half(), ins[1][0]], prs, ms)
    with pytest.raises(ValueError, match='float32.*float16.*bfloat16'):
        eng.run(ins[0][0].double(), prs[0], ms[0])
    with pytest.raises(ValueError, match='float32.*float16.*bfloat16'):
        eng.run_batch(torch.cat([ins[0][0], ins[1][0]]).to(torch.int32), prs, ms)
    eng.pe_rows_in_waves = True                                  # the opt-in second PE kernel has no 16-bit-map instance
    with pytest.raises(ValueError, match='pe_rows_in_waves'):
        eng.run(ins[0][0].half(), prs[0], ms[0])
    _snap(eng, eng.run(ins[0][0], prs[0], ms[0]))                # ... and keeps working on fp32 maps


# ---------------------------------------------------------------------------------------------------------- 5. plugin
def _build(kind, use_denoise=None, train=False):
    import mv2d_amd
    cfg = configs.roi_head_cfg_s() if kind == 'S' else configs.roi_head_cfg_t()
    if use_denoise is not None:
        cfg['use_denoise'] = use_denoise
    head = mv2d_amd.build_head(cfg, train_cfg=configs.TRAIN_CFG_RCNN if train else None, test_cfg=configs.TEST_CFG_RCNN)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_head_state(seed=0).items()}, strict=not train)
    return head.to(DEV)


def _spy(eng, seen):
    """Record the dtype of the map the engine receives."""
    for nm in ('run', 'run_batch'):
        def wrap(fn):
            def inner(feat, *a, **k):
                seen.append(feat.dtype if torch.is_tensor(feat) else [t.dtype for t in feat])
                return fn(feat, *a, **k)
            return inner
        setattr(eng, nm, wrap(getattr(eng, nm)))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('kind,name', [('S', 'cfg1_s'), ('T', 'cfg1_t')])
def test_plugin_simple_test_16bit_map(kind, name, dtype):
    from mv2d_amd import postprocess
    head = _build(kind).eval()
    probs = [synthetic.make_problem(name, seed=s) for s in (0, 4)]
    x16 = [torch.from_numpy(p['feat']).to(DEV).to(dtype) for p in probs]
    metas = [[dict(m, box_type_3d=None) for m in p['img_metas']] for p in probs]
    props = [[torch.from_numpy(x) for x in p['proposals']] for p in probs]
    want = [[t.clone() for t in head.simple_test([x16[b].float()], props[b], metas[b])[0]] for b in range(2)]
    seen = []
    _spy(head._engine, seen)
    for b in range(2):
        got = head.simple_test([x16[b]], props[b], metas[b])[0]
        assert all(same(x, y) for x, y in zip(got, want[b])) and len(got[2]) > 0
    gotb = head.simple_test_batch([torch.cat(x16)], props, metas)
    for b in range(2):
        assert all(same(x, y) for x, y in zip(gotb[b], want[b]))
    assert seen == [dtype, dtype, dtype]
    # the detection-side helpers hand the map on in its own dtype too
    seen.clear()
    dets = [[[x[x[:, 5] == c][:, :5] for c in range(10)] for x in p['proposals']] for p in probs]
    for up in (lambda x: x.float(), lambda x: x):
        one = postprocess.simple_test_from_detections(head, [up(x16[0])], dets[0], metas[0], configs.TEST_CFG_RCNN)[0]
        both = postprocess.simple_test_batch_from_detections(head, [up(torch.cat(x16))], dets, metas, configs.TEST_CFG_RCNN)
        if seen[-1] == torch.float32:
            want_one, want_both = one, both
    for k in ('boxes_3d', 'scores_3d', 'labels_3d'):
        assert same(one[k], want_one[k]) and all(same(both[b][k], want_both[b][k]) for b in range(2)), k
    assert seen == [torch.float32, torch.float32, dtype, dtype]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('with_dn', [False, True])
def test_forward_train_16bit_map_both_routes(with_dn, dtype):
    from test_gpu_roi_size import _dropout_off
    G, seed = 9, 31
    head = _dropout_off(_build('S', use_denoise=with_dn, train=True))
    prob = synthetic.make_problem('cfg1_s', seed=0)
    gtc = synthetic.make_train_gt(G, seed)
    rnd_ = torch.from_numpy(synthetic.make_dn_noise(G * 10, seed)).to(DEV)
    props = [torch.from_numpy(p) for p in prob['proposals']]
    metas = [dict(m, box_type_3d=None) for m in prob['img_metas']]
    gt_list, lab_list = [torch.from_numpy(gtc['gt'])], [torch.from_numpy(gtc['gt_labels'])]
    x16 = torch.from_numpy(prob['feat']).to(DEV).to(dtype)
    seen = []

    def losses_of(feat, autograd):
        head.zero_grad(set_to_none=True)
        if autograd:
            return head.forward_train([feat], metas, props, None, None, None, None, gt_list, lab_list, None, dn_noise=rnd_, autograd=True)
        with torch.no_grad():
            return head.forward_train([feat], metas, props, None, None, None, None, gt_list, lab_list, None, dn_noise=rnd_, autograd=False)
    for autograd in (False, True):
        want = {k: float(v.detach()) for k, v in losses_of(x16.float(), autograd).items()}
        if not seen:
            _spy(head._engine, seen)
            seen.clear()
        feat = x16.clone().requires_grad_(True)
        got = losses_of(feat, autograd)
        assert seen[-1] == dtype
        assert set(got) == set(want) and (any('dn_loss' in k for k in want) == with_dn)
        for k in want:
            assert np.isfinite(want[k]) and float(got[k].detach()) == want[k], (autograd, k, float(got[k].detach()), want[k])
        if autograd:
            sum(got.values()).backward()
            assert feat.grad is not None and feat.grad.dtype == dtype and feat.grad.shape == feat.shape
            assert bool(torch.isfinite(feat.grad).all()) and float(feat.grad.float().norm()) > 0


# ---------------------------------------------------------------------------------------------------------- 6. full size
@pytest.mark.parametrize('name', ['cfg2_s', 'cfg3_t'])
def test_full_size_sample_fp16_map(name):
    prob = synthetic.make_problem(name, seed=0)
    f, pr, m = _inputs(prob)
    assert tuple(f.shape[2:]) == (32, 88)                        # the stride-16 map of a 1408 x 512 image
    x16 = f.to(torch.float16)
    eng = _engine(prob)
    want = _snap(eng, eng.run(x16.float(), pr, m))
    out = eng.run(x16, pr, m)
    assert out['ws']['featcl'].dtype == torch.float16
    got = _snap(eng, out)
    n = int(want['count'][0])
    assert n > 0 and int(got['count'][0]) == n
    assert torch.equal(got['labels'][:n], want['labels'][:n]) and torch.equal(got['bbox_index'][:n], want['bbox_index'][:n])
    _assert_same(got, want)
