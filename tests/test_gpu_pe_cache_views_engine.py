"""Route option pe_cache_views in the engine (mv2d_amd/pe_cache.py PeViewCachePolicy, csrc/pe_x3_sel.h, csrc/pe_x3_gate.hip): on the two-frame head the
views whose camera matrices repeat (the current frame of a fixed calibration) read their slice of the cached frustum MLP and run the gate alone, the
views that carry the ego motion run the full kernel.  Two engines on the same weights, one with pe_cache_views = True: every output and the key / value
rows of every frame are bit for bit the same, whatever the sequence of matrices, batches, map formats, depths and weights.

The problem: 2 cameras x 2 frames of 128 x 192 pixels -- 4 views of 8 x 12 cells; `ego` moves only the previous-frame views (2, 3)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from mv2d_amd import synthetic
from test_gpu_pe_cache_engine import _moved

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OUT_KEYS = ('boxes', 'scores', 'labels', 'bbox_index', 'count', 'cls', 'reg')
ROW_KEYS = ('Xk', 'xk_lo', 'Xf_b', 'xv_lo')
H, W = 128, 192


def _metas(ego):
    return synthetic.make_img_metas(2, H, W, frames=2, yaw_step_deg=40.0, ego=ego)


_DATA = {}


def _data(seed):
    """(feature map [4,256,8,12], proposals) of one frame: built once per seed, never written"""
    if seed not in _DATA:
        _DATA[seed] = (torch.from_numpy(synthetic.make_feat(4, H // 16, W // 16, seed + 2)),
                       [torch.from_numpy(p) for p in synthetic.make_proposals(4, 6, H, W, seed + 1)])
    return _DATA[seed]


def _engines(sd=None, kind='T', **kw):
    from mv2d_amd.engine import HeadEngine
    sd = synthetic.make_head_state(seed=0) if sd is None else sd
    engs = [HeadEngine(sd, kind, torch.device(DEV), num_views=2, **kw) for _ in range(2)]
    assert engs[0].pe_cache_views is False                        # the default
    engs[0].pe_cache_views = True
    return engs


def _frame(engs, feat, props, metas, use_graph=False, batch=False):
    """one frame through both engines: equal bits everywhere; returns the output of the caching engine"""
    outs = []
    for e in engs:
        o = (e.run_batch if batch else e.run)(feat, props, metas, use_graph=use_graph)
        torch.cuda.synchronize()
        outs.append(o)
    a, b = outs
    assert b['pe_cache'] == 'off' and b['pe_cache_views'] == ()
    for k in OUT_KEYS:
        assert torch.equal(a[k], b[k]), k
    S = int(a['ws']['S_dev'].item())
    assert S == int(b['ws']['S_dev'].item()) and S > 0
    for k in ROW_KEYS:
        ra, rb = a['ws'][k][:S], b['ws'][k][:S]
        assert torch.equal(ra.view(torch.uint8), rb.view(torch.uint8)), k
    assert int(a['count'].sum()) > 0
    return a


@pytest.mark.parametrize('use_graph', [False, True])
def test_a_moving_vehicle_then_a_standing_one_then_another_rig(use_graph):
    engs = _engines()
    feat = torch.empty((4, 256, H // 16, W // 16), device=DEV)    # (one static input buffer: a captured graph holds its address)
    got = []
    seq = [0.0, 0.1, 0.2, 0.3, 0.3, 0.3]
    for i, ego in enumerate(seq):
        f, props = _data(i % 3)
        feat.copy_(f)
        out = _frame(engs, feat, props, _metas(ego), use_graph=use_graph)
        got.append((out['pe_cache'], out['pe_cache_views']))
        if i == 3:
            assert engs[0].pe_cache_builds == 1
    assert got == [('miss', ()), ('build', (0, 1)), ('hit', (0, 1)), ('hit', (0, 1)), ('build', (0, 1, 2, 3)), ('hit', (0, 1, 2, 3))]
    assert engs[0].pe_cache_builds == 2 and getattr(engs[1], 'pe_cache_builds', 0) == 0
    if use_graph:
        cur, parked = out['ws']['graphs'], out['ws']['graphs_other_pe_form']   # one graph of each form, whatever the mask was: the split form in use
        assert len(cur) == 1 and len(parked) == 1 and list(cur) == list(parked)
        assert [g[2] for g in cur.values()] == [True] and [g[2] for g in parked.values()] == [False]
    out = _frame(engs, feat, props, _moved(_metas(0.3), 0.25), use_graph=use_graph)      # the whole rig shifted
    assert (out['pe_cache'], out['pe_cache_views']) == ('miss', ())
    assert tuple(out['ws']['shared']['pe_q'].shape) == (4 * 8 * 12, 256)


def test_views_that_change_every_frame_never_build_and_never_call_the_new_entries(monkeypatch):
    from mv2d_amd import ops
    calls = []
    real_gate, real_full, real_frustum = ops.pe_gate_rows_x3, ops.pe_fused_x3, ops.pe_frustum_f32
    monkeypatch.setattr(ops, 'pe_gate_rows_x3', lambda *a, **k: (calls.append('gate'), real_gate(*a, **k))[1])
    monkeypatch.setattr(ops, 'pe_fused_x3', lambda *a, **k: (calls.append('full') if k.get('view_mask') is not None else None, real_full(*a, **k))[1])
    monkeypatch.setattr(ops, 'pe_frustum_f32', lambda *a, **k: (calls.append('frustum') if k.get('view_mask') is not None else None, real_frustum(*a, **k))[1])
    engs = _engines()
    for i in range(5):
        f, props = _data(i % 3)
        out = _frame(engs, f.to(DEV), props, _moved(_metas(0.1 * i), 0.01 * (i + 1)))
        assert (out['pe_cache'], out['pe_cache_views']) == ('miss', ())
    assert not calls and getattr(engs[0], 'pe_cache_builds', 0) == 0 and 'pe_q' not in out['ws']['shared']
    # ... and the counters do see the three launches of a frame that reads the table
    for _ in range(2):
        out = _frame(engs, f.to(DEV), props, _metas(0.0))
    assert out['pe_cache'] == 'build' and calls == ['frustum', 'full', 'gate']


def test_batches():
    engs = _engines()
    feats = [_data(s)[0].to(DEV) for s in (0, 1)]
    props = [_data(s)[1] for s in (0, 1)]
    for i, want in enumerate([('miss', ()), ('build', (0, 1)), ('hit', (0, 1))]):        # two samples of one rig: the slices of ONE sample serve both
        m = _metas(0.1 * i)
        out = _frame(engs, feats, props, [m, m], batch=True)
        assert (out['pe_cache'], out['pe_cache_views']) == want
    sh = out['ws']['shared']
    assert sh['pe_q'].shape[0] == sh['sine_period'] == out['ws']['P'] // 2
    assert int(out['count'][0]) > 0 and int(out['count'][1]) > 0
    builds = engs[0].pe_cache_builds
    for i in range(3):                                            # differing current-view matrices: those views stay uncached (and ego moves the others)
        m = _metas(0.5 + 0.1 * i)
        out = _frame(engs, feats, props, [m, _moved(m, 0.5)], batch=True)
        assert (out['pe_cache'], out['pe_cache_views']) == ('miss', ())
    assert engs[0].pe_cache_builds == builds
    # the samples differ in ONE current view only and the vehicle stands: the other three views are cached
    m = _metas(0.9)
    m2 = [m[0]] + _moved(m[1:2], 0.5) + m[2:]
    for want in (('miss', ()), ('build', (0, 2, 3)), ('hit', (0, 2, 3))):
        out = _frame(engs, feats, props, [m, m2], batch=True)
        assert (out['pe_cache'], out['pe_cache_views']) == want


@pytest.mark.parametrize('config', ['fp16_map', 'depth_40'])
def test_other_configurations_hit(config):
    kw, sd = {}, None
    if config == 'depth_40':
        sd, kw = synthetic.with_pe_depth_state(synthetic.make_head_state(seed=0), 0, 40), dict(depth_num=40)
    engs = _engines(sd=sd, **kw)
    feat, props = _data(0)
    feat = feat.to(DEV)
    if config == 'fp16_map':
        feat = feat.half()
    for i, want in enumerate([('miss', ()), ('build', (0, 1)), ('hit', (0, 1))]):
        out = _frame(engs, feat, props, _metas(0.1 * i))
        assert (out['pe_cache'], out['pe_cache_views']) == want


def test_new_weights_rebuild_the_slices():
    from mv2d_amd.engine import HeadEngine
    sd2 = synthetic.make_head_state(seed=1)
    engs = _engines()
    feat, props = _data(0)
    feat = feat.to(DEV)
    for i, want in enumerate(['miss', 'build', 'hit']):
        assert _frame(engs, feat, props, _metas(0.1 * i))['pe_cache'] == want
    engs[0].load_state(sd2)
    fresh = HeadEngine(sd2, 'T', torch.device(DEV), num_views=2)
    for i, want in enumerate([('miss', ()), ('build', (0, 1)), ('hit', (0, 1))]):
        out = _frame([engs[0], fresh], feat, props, _metas(0.3 + 0.1 * i))
        assert (out['pe_cache'], out['pe_cache_views']) == want
    assert engs[0].pe_cache_builds == 2


def test_hit_frame_against_the_reference_golden():
    """micro_t (one frame of two views: both repeat) with the option on: its third frame reads the table for every row; against
    tests/golden/micro_t.npz under the bounds of test_gpu_golden.py::test_exact_mode_integer_outputs_equal_the_reference."""
    from mv2d_amd.engine import HeadEngine
    from test_gpu_golden import index_mismatches, rel
    g = load_golden('micro_t')
    prob = synthetic.make_problem('micro_t', seed=0)
    eng = HeadEngine(synthetic.make_head_state(seed=0), 'T', torch.device(DEV), num_views=prob['views_per_frame'], exact=True)
    eng.pe_cache_views = True
    feat = torch.from_numpy(prob['feat']).to(DEV)
    props = [torch.from_numpy(np.asarray(p)) for p in prob['proposals']]
    for want in ('miss', 'build', 'hit'):
        out = eng.run(feat, props, prob['img_metas'])
        torch.cuda.synchronize()
        assert out['pe_cache'] == want
    assert out['pe_cache_views'] == (0, 1)
    R = out['R']
    n_lab, n_idx, n_set, tot = index_mismatches(out, g)
    e_cls = rel(out['cls'][:, :R].reshape(g['cls'].shape), g['cls'])
    e_sc = rel(out['scores'][:tot], g['scores'])
    print(f'[pe_cache_views] micro_t hit frame: {n_lab}/{tot} ranked labels, {n_idx}/{tot} ranked indices differ; cls rel err {e_cls:.1e}, score rel err {e_sc:.1e}')
    assert e_cls < 3e-6 and e_sc < 1e-5
    assert n_lab == 0 and n_idx in (0, None) and n_set in (0, None)


def test_the_single_frame_head_ignores_the_option():
    """An S engine with the option on behaves as with it off: its own cache (pe_cache), the same bits, none of the new entries."""
    from mv2d_amd.engine import HeadEngine
    prob = synthetic.make_problem('micro_s', seed=0)
    sd = synthetic.make_head_state(seed=0)
    engs = [HeadEngine(sd, 'S', torch.device(DEV), num_views=prob['views_per_frame']) for _ in range(2)]
    engs[0].pe_cache_views = True
    feat = torch.from_numpy(prob['feat']).to(DEV)
    props = [torch.from_numpy(np.asarray(p)) for p in prob['proposals']]
    for want in ('miss', 'build', 'hit'):
        a, b = [e.run(feat, props, prob['img_metas']) for e in engs]
        torch.cuda.synchronize()
        assert a['pe_cache'] == b['pe_cache'] == want and a['pe_cache_views'] == b['pe_cache_views'] == ()
        for k in OUT_KEYS:
            assert torch.equal(a[k], b[k]), k
        assert torch.equal(a['ws']['pe_pos'], b['ws']['pe_pos'])
    assert 'pe_qv_policy' not in a['ws']['shared'] and 'pe_vmask' not in a['ws']['shared']
