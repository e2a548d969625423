"""The block dealing of the one-launch cross attention only moves WHICH BLOCK computes a query, never how it is computed: every deal the wrapper can
force gives the bits of every other one (compared on the bit patterns; a NaN only where the other has one).

    ops.xattn_fused(deal=...)   csrc/xattn_fused.hip: a launch of more blocks of 8 queries than the chip has CUs is cut into whole rounds of CUs
                                (deal 1: blocks of 4 .. 8 queries) or into ceil(R / 8) full blocks (deal 2, the library's policy, deal 0).
                                R = 2049, 2056, 2305 are 257, 257 and 289 blocks of 8 -- one query over 256 blocks, every block full, a remainder of
                                one -- all beyond the 256 CUs of an MI355X, which is where the dealing branch starts.  Rows of 0 .. 3 keys out of
                                a 64-row key table (empty rows with both empty_nan values), hi + e4m3 lo rows, key16 lo rows, a launch order;
                                outputs in front of guard rows.  Also held to the three-kernel path (xattn_qmap, xattn_tile with one wave per
                                query, xattn_ctxmap).
    HeadEngine.xattn_deal       one micro_s frame, eager and through a captured graph, with the deal forced through the wrapper's argument: every
                                output of the frame, and the argument the wrapper receives.

The default path never forces a deal: Route.xattn_deal = 0 unless the option is set (first test, needs no GPU)."""
import functools

import numpy as np
import pytest
import torch

DEV = 'cuda:0'
SENTINEL = -12345.0
GUARD_ROWS = 64
XF_KEYS = 64


def test_default_route_forces_no_deal():
    from types import SimpleNamespace

    from mv2d_amd import route
    assert route.default_options()['xattn_deal'] == 0
    for kind in ('S', 'T'):
        r = route.resolve(SimpleNamespace(**route.default_options()), kind, True, 64)
        assert r.xattn_deal == 0 and 'xattn_deal' not in route.Storage._fields
        forced = route.resolve(SimpleNamespace(**dict(route.default_options(), xattn_deal=1)), kind, True, 64)
        assert forced.xattn_deal == 1 and forced.storage == r.storage and forced != r
    with pytest.raises(ValueError, match='xattn_deal'):
        route.resolve(SimpleNamespace(**dict(route.default_options(), xattn_deal=3)), 'S', True, 64)


def _bits(a, b):
    """NaN in the same places, the same bits elsewhere"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a.masked_fill(na, 0.0).view(torch.int32), b.masked_fill(nb, 0.0).view(torch.int32))


def _guarded(rows, width):
    buf = torch.full(((rows + GUARD_ROWS) * width,), SENTINEL, device=DEV, dtype=torch.float32)
    return buf, buf[:rows * width].view(rows, width)


def _intact(buf, n):
    return bool((buf[n:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ cross attention
def _randn(seed, shape, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _xf_tables():
    """what does not depend on R: the key table (hi + key16 lo, and the lo halves as e4m3 bytes), the packed maps"""
    from mv2d_amd import ops
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    Xk, Xk_lo = ops.f32_to_key16(_randn(7101, (XF_KEYS, 256)).to(DEV), with_lo=True)
    Xv, Xv_lo = ops.f32_to_key16(_randn(7102, (XF_KEYS, 256)).to(DEV), with_lo=True)
    WA, WB = ops.pack_xattn_maps(_randn(7103, (256, 256), 0.06).to(DEV), _randn(7104, (256, 256), 0.06).to(DEV))
    return dict(Xk=Xk, Xv=Xv, lo16=(Xk_lo, Xv_lo), lo8=(ops.lo8_encode(Xk_lo), ops.lo8_encode(Xv_lo)), WA=WA, WB=WB, bv=_randn(7105, (256,)).to(DEV))


@functools.lru_cache(maxsize=None)
def _xf_rows(R):
    """queries and a CSR of 0 .. 3 distinct keys per row; rows 0, 7, R - 8 and R - 1 are empty and rows 1 and R - 2 hold 3 keys whatever was drawn"""
    g = np.random.Generator(np.random.PCG64(7200 + R))
    nk = g.integers(0, 4, R)
    nk[[0, 7, R - 8, R - 1]] = 0
    nk[[1, R - 2]] = 3
    row_ptr = np.concatenate([[0], np.cumsum(nk)]).astype(np.int32)
    col = np.concatenate([g.choice(XF_KEYS, n, replace=False) for n in nk]).astype(np.int32)
    return dict(q=(_randn(7300 + R, (R, 256)) * 0.3).to(DEV), row_ptr=torch.from_numpy(row_ptr).to(DEV), col=torch.from_numpy(col).to(DEV),
                empty=torch.from_numpy(nk == 0).to(DEV))


@functools.lru_cache(maxsize=None)
def _xf_three_kernels(R, lo, empty_nan):
    from mv2d_amd import ops
    t, r = _xf_tables(), _xf_rows(R)
    Qt = ops.xattn_qmap(r['q'], t['WA'])
    z = ops.xattn_tile(Qt, t['Xk'], t['Xv'], r['row_ptr'], r['col'], empty_nan=empty_nan, waves=1, Xk_lo=t[lo][0], Xv_lo=t[lo][1])
    return ops.xattn_ctxmap(z, t['WB'], t['bv'], r['row_ptr'], empty_nan=empty_nan)


@pytest.mark.gpu
@pytest.mark.parametrize('R,lo,ordered', [(2049, 'lo8', False), (2056, 'lo8', False), (2305, 'lo8', False), (2056, 'lo16', False), (2305, 'lo8', True)])
def test_xattn_fused_deals_are_the_same_rows(R, lo, ordered):
    from mv2d_amd import ops
    t, r = _xf_tables(), _xf_rows(R)
    assert torch.cuda.get_device_properties(0).multi_processor_count < (R + 7) // 8, 'the dealing branch needs more blocks of 8 than CUs'
    order = torch.randperm(R, generator=torch.Generator().manual_seed(R)).to(torch.int32).to(DEV) if ordered else None
    for empty_nan in (True, False):
        want = _xf_three_kernels(R, lo, empty_nan)
        got = {}
        for deal in (1, 2, 0):
            buf, out = _guarded(R, 256)
            ops.xattn_fused(r['q'], t['WA'], t['WB'], t['bv'], t['Xk'], t['Xv'], r['row_ptr'], r['col'], out=out, R=R, empty_nan=empty_nan,
                            Xk_lo=t[lo][0], Xv_lo=t[lo][1], order=order, deal=deal)
            torch.cuda.synchronize()
            assert _intact(buf, R * 256), (deal, empty_nan)
            got[deal] = out
        assert _bits(got[2], got[1]), ('deal 2 against deal 1', empty_nan)
        assert _bits(got[2], want), ('deal 2 against the three kernels', empty_nan)
        assert _bits(got[0], want), ('the default deal against the three kernels', empty_nan)
        rows_nan = torch.isnan(got[2]).all(1)
        assert torch.equal(rows_nan, r['empty'] if empty_nan else torch.zeros_like(r['empty']))
        if not empty_nan:
            assert bool((got[2][r['empty']] == 0).all())
    with pytest.raises(Exception):
        ops.xattn_fused(r['q'], t['WA'], t['WB'], t['bv'], t['Xk'], t['Xv'], r['row_ptr'], r['col'], R=R, deal=3)


# ------------------------------------------------------------------------------------------------ engine
@pytest.mark.gpu
def test_engine_frame_with_a_forced_deal_equals_the_default(monkeypatch):
    """micro_s with xattn_deal = 1 and 2 handed through the wrapper's forcing argument (Route.xattn_deal): the wrapper receives it in every layer, and
    every tensor the frame returns, eager and through a captured graph, is bit for bit the default's; a forced route captures a graph of its own on
    the same buffers."""
    from mv2d_amd import ops, synthetic
    from mv2d_amd.engine import HeadEngine
    prob = synthetic.make_problem('micro_s', seed=0)
    dev = torch.device(DEV)
    eng = HeadEngine(synthetic.make_head_state(seed=0), 'S', dev, num_views=prob['views_per_frame'])
    feat = torch.from_numpy(prob['feat']).to(dev)
    props = [torch.from_numpy(p) for p in prob['proposals']]
    seen, real = [], ops.xattn_fused

    def spy(*a, **kw):
        seen.append(kw.get('deal', 0))
        return real(*a, **kw)
    monkeypatch.setattr(ops, 'xattn_fused', spy)

    def frames():
        outs = []
        for use_graph in (False, True):
            o = eng.run(feat, props, prob['img_metas'], use_graph=use_graph)
            torch.cuda.synchronize()
            outs.append({k: v.clone() for k, v in o.items() if isinstance(v, torch.Tensor)})
        return outs

    assert eng.xattn_deal == 0
    want = frames()
    assert seen and set(seen) == {0}
    assert {'cls', 'reg', 'boxes', 'scores', 'labels', 'bbox_index', 'count'} <= set(want[0])
    for deal in (1, 2):
        del seen[:]
        eng.xattn_deal = deal
        got = frames()
        assert seen and set(seen) == {deal}
        for g, w, mode in zip(got, want, ('eager', 'graph')):
            assert set(g) == set(w)
            for k in w:
                same = _bits(g[k], w[k]) if w[k].dtype == torch.float32 else torch.equal(g[k], w[k])
                assert same, (deal, mode, k)
    assert len(eng._ws_base) == 1                   # a launch-only option: the same buffers
