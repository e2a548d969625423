"""The view filter of the split-precision PE kernels (two-frame head, route option pe_cache_views; csrc/pe_x3_sel.h): the gate kernel with key / value
row outputs on a cached frustum MLP (pe_x3_gate_rows_kernel, mv2d_pe_gate_rows_x3) writes the rows of the views whose mask bit is set, the filtered full
kernel (pe_x3_sel_kernel, mv2d_pe_fused_x3_k_sel) the others, and together they leave BIT FOR BIT what one unfiltered ops.pe_fused_x3 launch writes:
Xk hi / lo, Xv hi / lo, both lo formats, the lo8 flag word, the three map formats.  Weights and Q are built as in tests/test_gpu_pe_gate.py::_case.

The map: 4 views of 6 x 8 cells, two samples -- hw = 48, tab_period = 192, 384 positions; 48 is no multiple of the 64-row tile, so tiles straddle view
and sample edges."""
import numpy as np
import pytest
import torch

from test_gpu_pe_gate import _kp, rnd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
VIEWS, HW = 4, 48
PERIOD, NPOS = VIEWS * HW, 2 * VIEWS * HW
FILL = 0x5A                                 # sentinel byte of every output buffer
MASKS = [0x0, 0x1, 0x5, 0xA, 0xF]
NAMES = ('Xk_hi', 'Xk_lo', 'Xv_hi', 'Xv_lo', 'flag')

_CASE = {}


def _case(D):
    """Weights, biases, table, the frustum rows of the PERIOD positions of one sample, the feature map (a few values of +-300.12: the fp16 grid is 0.25 wide there, the lo
    remainder 0.12 * 2^12 leaves the e4m3 range and raises the lo8 flag; 300.0 itself is an fp16 number with remainder 0) and Q for one depth: built once, shared by the tests, never written."""
    if D not in _CASE:
        from mv2d_amd import ops
        W = dict(w1a=rnd((1024, 3 * D), 193 + D, 0.08 * (192.0 / (3 * D)) ** 0.5), w1b=rnd((256, 1024), 194, 0.04), wr=rnd((256, 256), 197, 0.07),
                 we=rnd((256, 256), 198, 0.07))
        wx = {k: ops.pack_x3(ops.pad_pe_w1a(v.to(DEV), D) if k == 'w1a' else v.to(DEV)) for k, v in W.items()}
        wx.update({k: rnd((n,), 199 + i).to(DEV) for i, (k, n) in enumerate(dict(b1a=1024, b1b=256, br=256, be=256).items())})
        tab = rnd((PERIOD, 256), 231).to(DEV)
        A1 = torch.zeros((PERIOD, _kp(D)), device=DEV)
        A1[:, :3 * D] = (rnd((PERIOD, 3 * D), 190 + D) * 3.0).to(DEV)
        Xmap = rnd((NPOS, 256), 192)
        for i, (r, c) in enumerate(((3, 7), (50, 100), (97, 255), (150, 0), (200, 31), (290, 64), (340, 200), (383, 129))):      # every view of both samples
            Xmap[r, c] = 300.12 * (-1) ** i
        Q = torch.empty((PERIOD, 256), device=DEV)
        ops.pe_fused_x3(A1, None, None, wx, torch.zeros((1, 256), device=DEV), 1, pe=Q, M=PERIOD, Kp=_kp(D), gate=False)
        _CASE[D] = dict(wx=wx, tab=tab, A1=A1, Xmap=Xmap.to(DEV), Q=Q)
    return _CASE[D]


def _rows(M, order, seed=6):
    """M distinct map positions of both samples, in ascending order (the T path's key list) or permuted"""
    pos = torch.randperm(NPOS, generator=torch.Generator().manual_seed(seed))[:M]
    return (pos.sort().values if order == 'sorted' else pos).to(torch.int32).to(DEV)


def _bufs(M, lo_fmt):
    from mv2d_amd import ops
    k16 = ops.key16_dtype()
    b = dict(Xk_hi=torch.empty((M, 256), dtype=k16, device=DEV), Xv_hi=torch.empty((M, 256), dtype=k16, device=DEV),
             Xk_lo=torch.empty((M, 256), dtype=torch.uint8 if lo_fmt else k16, device=DEV),
             Xv_lo=torch.empty((M, 256), dtype=torch.uint8 if lo_fmt else k16, device=DEV), flag=torch.zeros(1, dtype=torch.int32, device=DEV))
    for n in NAMES[:4]:
        b[n].view(torch.uint8).fill_(FILL)
    return b


def _raw(t):
    return t.view(torch.uint8).reshape(t.shape[0], -1)


def _full(c, D, ri, M, b, md=None, Xmap=None, mask=None):
    """the full kernel on the frustum rows of the listed positions: unfiltered, or (mask: device word) the rows of the clear views only"""
    from mv2d_amd import ops
    A1 = c['A1'][ri.long() % PERIOD].contiguous()
    sel = {} if mask is None else dict(view_mask=mask, hw=HW)
    ops.pe_fused_x3(A1, c['Xmap'] if Xmap is None else Xmap, md, c['wx'], c['tab'], PERIOD, Xk=(b['Xk_hi'], b['Xk_lo']), Xv=(b['Xv_hi'], b['Xv_lo']), M=M,
                    row_index=ri, lo8_flag=b['flag'], Kp=_kp(D), **sel)


def _gate(c, ri, M, b, mask, md=None, Xmap=None):
    from mv2d_amd import ops
    ops.pe_gate_rows_x3(c['Q'], c['Xmap'] if Xmap is None else Xmap, md, c['wx'], c['tab'], PERIOD, (b['Xk_hi'], b['Xk_lo']), (b['Xv_hi'], b['Xv_lo']), M,
                        mask, HW, row_index=ri, lo8_flag=b['flag'])


def _word(m):
    return torch.tensor([m], dtype=torch.int32, device=DEV)


def _set(ri, m):
    """bool [M]: the rows whose view bit is set"""
    return ((m >> ((ri.long() % PERIOD) // HW)) & 1).bool()


def _assert_same(got, ref, what):
    for n in NAMES:
        assert torch.equal(_raw(got[n]) if n != 'flag' else got[n], _raw(ref[n]) if n != 'flag' else ref[n]), (what, n)


@pytest.mark.parametrize('M', [1, 63, 64, 65, 200, 384])
@pytest.mark.parametrize('m', MASKS)
def test_the_two_filtered_launches_equal_one_unfiltered_launch_bitwise(m, M):
    """One row, the tile edge from both sides, several tiles with a ragged tail, every position; sorted and permuted row lists; key16 and e4m3 lo rows
    (the +-300.12 features raise the lo8 flag in both).  Every row is written by exactly one of the two launches."""
    c = _case(64)
    for order in ('sorted', 'permuted'):
        ri = _rows(M, order)
        for lo_fmt in (0, 1):
            ref, got = _bufs(M, lo_fmt), _bufs(M, lo_fmt)
            _full(c, 64, ri, M, ref)
            _gate(c, ri, M, got, _word(m))
            _full(c, 64, ri, M, got, mask=_word(m))
            _assert_same(got, ref, (order, lo_fmt))
            assert bool((_raw(ref['Xk_hi']) != FILL).any(1).all())
            if lo_fmt and M == 384:
                assert int(ref['flag'].item()) == 1                       # (all eight +-300.12 values are listed)


@pytest.mark.parametrize('lo_fmt', [0, 1])
def test_each_launch_alone_leaves_the_other_rows_at_the_sentinel(lo_fmt):
    c, M, m = _case(64), 200, 0x5
    for order in ('sorted', 'permuted'):
        ri = _rows(M, order)
        ref, g, f = _bufs(M, lo_fmt), _bufs(M, lo_fmt), _bufs(M, lo_fmt)
        _full(c, 64, ri, M, ref)
        _gate(c, ri, M, g, _word(m))
        _full(c, 64, ri, M, f, mask=_word(m))
        s = _set(ri, m)
        assert 0 < int(s.sum()) < M
        for n in NAMES[:4]:
            assert torch.equal(_raw(g[n])[s], _raw(ref[n])[s]) and bool((_raw(g[n])[~s] == FILL).all()), (order, n)
            assert torch.equal(_raw(f[n])[~s], _raw(ref[n])[~s]) and bool((_raw(f[n])[s] == FILL).all()), (order, n)
    # take_set flips the class a launch writes: the full kernel on the SET views, the gate on the clear ones
    from mv2d_amd import ops
    f2, g2 = _bufs(M, lo_fmt), _bufs(M, lo_fmt)
    ops.pe_fused_x3(c['A1'][ri.long() % PERIOD].contiguous(), c['Xmap'], None, c['wx'], c['tab'], PERIOD, Xk=(f2['Xk_hi'], f2['Xk_lo']), Xv=(f2['Xv_hi'], f2['Xv_lo']),
                    M=M, row_index=ri, lo8_flag=f2['flag'], Kp=192, view_mask=_word(m), hw=HW, take_set=True)
    ops.pe_gate_rows_x3(c['Q'], c['Xmap'], None, c['wx'], c['tab'], PERIOD, (g2['Xk_hi'], g2['Xk_lo']), (g2['Xv_hi'], g2['Xv_lo']), M, _word(m), HW, row_index=ri,
                        lo8_flag=g2['flag'], take_set=False)
    for n in NAMES[:4]:
        assert torch.equal(_raw(f2[n]), _raw(g[n])) and torch.equal(_raw(g2[n]), _raw(f[n])), n


def test_device_side_row_count():
    """m_dev = 130 of M = 200 launched rows: rows past 130 are untouched by both launches."""
    c, M = _case(64), 200
    ri = _rows(M, 'sorted')
    md = torch.tensor([130], dtype=torch.int32, device=DEV)
    for m in (0x5, 0xF):
        ref, got = _bufs(M, 1), _bufs(M, 1)
        _full(c, 64, ri, M, ref, md=md)
        _gate(c, ri, M, got, _word(m), md=md)
        _full(c, 64, ri, M, got, md=md, mask=_word(m))
        _assert_same(got, ref, m)
        for n in NAMES[:4]:
            assert bool((_raw(got[n])[130:] == FILL).all()) and bool((_raw(got[n])[:130] != FILL).any(1).all())


@pytest.mark.parametrize('D', [64, 8])
@pytest.mark.parametrize('map_dtype', [torch.float32, torch.float16, torch.bfloat16])
def test_map_formats_and_depths(map_dtype, D):
    """fp32 / fp16 / bf16 maps; the filtered full kernel at Kp = 192 (64 bins) and Kp = 32 (8 bins), the gate kernel one instance for both."""
    c, M, m = _case(D), 200, 0xA
    x = c['Xmap'].to(map_dtype)
    ri = _rows(M, 'permuted')
    for lo_fmt in (0, 1):
        ref, got = _bufs(M, lo_fmt), _bufs(M, lo_fmt)
        _full(c, D, ri, M, ref, Xmap=x)
        _gate(c, ri, M, got, _word(m), Xmap=x)
        _full(c, D, ri, M, got, Xmap=x, mask=_word(m))
        _assert_same(got, ref, lo_fmt)


@pytest.mark.parametrize('Kp', [64, 96, 128, 160, 224, 256])
def test_the_filtered_full_kernel_at_every_other_depth(Kp):
    """the instances of the filtered full kernel that no engine test reaches: its rows against the unfiltered kernel of the same Kp (no Q needed)"""
    from mv2d_amd import ops
    c, M, m = _case(64), 130, 0x6
    D = Kp // 3
    w1a = ops.pack_x3(ops.pad_pe_w1a(rnd((1024, 3 * D), 300 + Kp, 0.08).to(DEV), D))
    wx = dict(c['wx'], w1a=w1a)
    ri = _rows(M, 'sorted')
    A1 = torch.zeros((M, Kp), device=DEV)
    A1[:, :3 * D] = (rnd((M, 3 * D), 400 + Kp) * 3.0).to(DEV)
    ref, got = _bufs(M, 1), _bufs(M, 1)
    for b, sel in ((ref, {}), (got, dict(view_mask=_word(m), hw=HW))):
        ops.pe_fused_x3(A1, c['Xmap'], None, wx, c['tab'], PERIOD, Xk=(b['Xk_hi'], b['Xk_lo']), Xv=(b['Xv_hi'], b['Xv_lo']), M=M, row_index=ri,
                        lo8_flag=b['flag'], Kp=Kp, **sel)
    s = _set(ri, m)
    assert 0 < int(s.sum()) < M
    for n in NAMES[:4]:
        assert torch.equal(_raw(got[n])[~s], _raw(ref[n])[~s]) and bool((_raw(got[n])[s] == FILL).all()), n


def test_a_nan_feature_of_a_cached_view_poisons_exactly_its_row():
    c, M, m = _case(64), 200, 0x5
    ri = _rows(M, 'sorted')
    s = _set(ri, m)
    row = int(torch.nonzero(s)[37])                                      # a row of a cached view, in the middle of a tile
    x = c['Xmap'].clone()
    x[int(ri[row]), 11] = float('nan')
    clean, ref, got = _bufs(M, 1), _bufs(M, 1), _bufs(M, 1)
    _full(c, 64, ri, M, clean)
    _full(c, 64, ri, M, ref, Xmap=x)
    _gate(c, ri, M, got, _word(m), Xmap=x)
    _full(c, 64, ri, M, got, Xmap=x, mask=_word(m))
    _assert_same(got, ref, 'nan')
    assert bool(torch.isnan(got['Xk_hi'][row].float()).all())            # the gate mixes all channels: the whole key row
    nan_v = torch.isnan(got['Xv_hi'][row].float())
    assert int(nan_v.sum()) == 1 and bool(nan_v[11])                     # the value row carries the one NaN
    others = torch.ones(M, dtype=torch.bool, device=DEV)
    others[row] = False
    for n in NAMES[:4]:
        assert torch.equal(_raw(got[n])[others], _raw(clean[n])[others]), n


def test_the_filtered_frustum_rows():
    """mv2d_pe_frustum_f32_sel writes exactly the rows of the clear views, equal to the unfiltered entry's, and leaves the others at the sentinel."""
    from mv2d_amd import calib, ops, synthetic
    from oracle import mv2d_oracle as O
    metas = synthetic.make_img_metas(2, 128, 192, frames=2, yaw_step_deg=40.0, ego=0.1)           # 4 views of 8 x 12 cells
    V, h, w = 4, 8, 12
    P, D, Kp = V * h * w, 64, 192
    ft = calib.frame_tables(metas, h, w, depth_num=D, depth_start=1, position_range=tuple(O.POST_RANGE))
    T = {k: ft[k].to(DEV) for k in ('img2lidar', 'coords_w', 'coords_h', 'coords_d')}
    pr = torch.tensor(list(O.POST_RANGE), dtype=torch.float64)
    g = np.random.Generator(np.random.PCG64(82))
    sel = g.choice(P, size=(2 * P) // 3, replace=False).astype(np.int32)          # a permuted list
    S = len(sel)
    s2pos, S_dev = torch.from_numpy(sel).to(DEV), torch.tensor([S - 5], dtype=torch.int32, device=DEV)
    ref = torch.full((P, Kp), float('nan'), device=DEV)
    ops.pe_frustum_f32(s2pos, S_dev, P, T['img2lidar'], T['coords_w'], T['coords_h'], T['coords_d'], ref, V, h, w, D, pr, ld=Kp)
    view = torch.from_numpy(sel).long().to(DEV) // (h * w)
    for m in MASKS:
        got = torch.full((P, Kp), float('nan'), device=DEV)
        ops.pe_frustum_f32(s2pos, S_dev, P, T['img2lidar'], T['coords_w'], T['coords_h'], T['coords_d'], got, V, h, w, D, pr, ld=Kp, view_mask=_word(m),
                           tab_period=P)
        clear = ((m >> view) & 1) == 0
        clear[S - 5:] = False                                                      # (past the device-side count: nobody's rows)
        assert torch.equal(got[:S][clear], ref[:S][clear]) and not bool(torch.isnan(got[:S][clear]).any())
        rest = torch.ones(P, dtype=torch.bool, device=DEV)
        rest[:S][clear] = False
        assert bool(torch.isnan(got[rest]).all())


def test_refusals_name_the_entry():
    from mv2d_amd import _lib, ops
    c, M = _case(64), 65
    ri = _rows(M, 'sorted')
    b = _bufs(M, 1)
    xk, xv = (b['Xk_hi'], b['Xk_lo']), (b['Xv_hi'], b['Xv_lo'])
    A1 = c['A1'][ri.long() % PERIOD].contiguous()
    gate = lambda mask=_word(1), hw=HW, period=PERIOD, Q=c['Q'], **kw: ops.pe_gate_rows_x3(Q, c['Xmap'], None, c['wx'], c['tab'], period, kw.pop('Xk', xk),  # noqa: E731
                                                                                        kw.pop('Xv', xv), M, mask, hw, row_index=ri, **kw)
    full = lambda mask=_word(1), hw=HW, period=PERIOD, **kw: ops.pe_fused_x3(A1, c['Xmap'], None, c['wx'], c['tab'], period, M=M, row_index=ri,  # noqa: E731
                                                                            view_mask=mask, hw=hw, **dict(dict(Xk=xk, Xv=xv, Kp=192), **kw))
    for fn, name in ((gate, 'mv2d_pe_gate_rows_x3'), (full, 'mv2d_pe_fused_x3_k_sel')):
        with pytest.raises(_lib.Mv2dHipError, match=name + '.*Vg <= 32'):                  # 384 / 8 = 48 views
            fn(hw=8, period=NPOS)
        with pytest.raises(_lib.Mv2dHipError, match=name + '.*tab_period % hw'):
            fn(hw=50)
        with pytest.raises(_lib.Mv2dHipError, match=name + '.*tab_period % hw'):
            fn(hw=None)
        with pytest.raises(_lib.Mv2dHipError, match=name + '.*view_mask.*expected torch.int32'):
            fn(mask=_word(1).long())
        with pytest.raises(_lib.Mv2dHipError, match=name + '.*view_mask.*on the GPU'):
            fn(mask=torch.tensor([1], dtype=torch.int32))
        with pytest.raises(_lib.Mv2dHipError, match=name + '.*one int32 word'):
            fn(mask=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_gate_rows_x3.*Xk and Xv are required'):
        gate(Xk=None)
    with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_gate_rows_x3.*tab_period = 96'):  # a Q of another period than stated
        gate(period=96)
    with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_gate_rows_x3.*Q.*expected torch.float32'):
        gate(Q=c['Q'].double())
    with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_gate_rows_x3.*pe.*expected torch.float32'):
        gate(pe=torch.zeros((M, 256), dtype=torch.float16, device=DEV))
    with pytest.raises(ValueError, match='accepted dtypes'):
        ops.pe_gate_rows_x3(c['Q'], c['Xmap'].double(), None, c['wx'], c['tab'], PERIOD, xk, xv, M, _word(1), HW, row_index=ri)
    with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_fused_x3_k_sel.*gated kernel with key / value row outputs'):
        full(Xk=None, Xv=None, pe=torch.zeros((M, 256), device=DEV))
    with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_fused_x3_k_sel.*gated kernel'):
        full(gate=False)
    with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_frustum_f32_sel.*tab_period % hw'):
        one = torch.zeros(4, dtype=torch.float64, device=DEV)
        ops.pe_frustum_f32(ri, _word(1), M, one, one, one, one, torch.zeros((M, 192), device=DEV), 8, 6, 8, 64, torch.zeros(6, dtype=torch.float64), ld=192,
                           view_mask=_word(1), tab_period=100)
    # the unfiltered gate entry stays as it is: it still refuses row pointers
    with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_gate_x3.*key / value row'):
        ops.pe_gate_x3(c['Q'], c['Xmap'], None, c['wx'], c['tab'], PERIOD, torch.zeros((M, 256), device=DEV), M, row_index=ri, Xk=xk, Xv=xv)
    assert bool((_raw(b['Xk_hi']) == FILL).all())                                           # nothing was launched
