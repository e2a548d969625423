"""Route option pe_cache in the engine (mv2d_amd/pe_cache.py, csrc/pe_x3_gate.hip): on a rig whose camera matrices repeat, the frustum MLP of the PE
is built once and a frame runs the gate alone.  Two engines on the same weights, one with pe_cache = False: every output of every frame is bit for
bit the same, whatever the sequence of matrices, weights, batches, map formats and depths; streams whose matrices always change never build."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from mv2d_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OUT_KEYS = ('boxes', 'scores', 'labels', 'bbox_index', 'count', 'cls', 'reg')


def _engine(prob, sd=None, cache=True, **kw):
    from mv2d_amd.engine import HeadEngine
    eng = HeadEngine(synthetic.make_head_state(seed=0) if sd is None else sd, prob['kind'], torch.device(DEV), num_views=prob['views_per_frame'], **kw)
    assert eng.pe_cache is True                                   # the default
    eng.pe_cache = cache
    return eng


def _props(prob):
    return [torch.from_numpy(np.asarray(p)) for p in prob['proposals']]


def _moved(metas, dx):
    """the rig with every camera shifted by dx metres: other extrinsics and lidar2img"""
    out = []
    for m in metas:
        T = np.asarray(m['extrinsics']).T.copy()
        T[:3, 3] += [dx, 0.0, 0.0]
        out.append(dict(m, extrinsics=T.T.copy(), lidar2img=np.asarray(m['intrinsics']) @ T))
    return out


def _frame(engs, feat, props, metas, use_graph=False, batch=False):
    """one frame through both engines: equal bits everywhere; returns (state of the caching engine, its output)"""
    outs = []
    for e in engs:
        o = (e.run_batch if batch else e.run)(feat, props, metas, use_graph=use_graph)
        torch.cuda.synchronize()
        outs.append(o)
    a, b = outs
    assert b['pe_cache'] == 'off'
    for k in OUT_KEYS:
        assert torch.equal(a[k], b[k]), k
    assert a['ws']['pe_pos'] is not None and torch.equal(a['ws']['pe_pos'], b['ws']['pe_pos'])
    assert float(a['ws']['pe_pos'].abs().sum()) > 0
    return a['pe_cache'], a


PROBS = {}


def _prob(name, seed):
    if (name, seed) not in PROBS:
        PROBS[name, seed] = synthetic.make_problem(name, seed=seed)
    return PROBS[name, seed]


@pytest.mark.parametrize('use_graph', [False, True])
def test_hit_path_is_bitwise_the_full_kernel(use_graph):
    """Four frames with the same metas, other features and boxes: miss, build, hit, hit."""
    probs = [_prob('micro_s', s) for s in range(4)]
    engs = [_engine(probs[0]), _engine(probs[0], cache=False)]
    feat = torch.empty(probs[0]['feat'].shape, device=DEV)        # (one static input buffer: a captured graph holds its address)
    states = []
    for p in probs:
        feat.copy_(torch.from_numpy(p['feat']))
        state, out = _frame(engs, feat, _props(p), p['img_metas'], use_graph=use_graph)
        states.append(state)
    assert states == ['miss', 'build', 'hit', 'hit'] and engs[0].pe_cache_builds == 1
    if use_graph:
        cur, parked = out['ws']['graphs'], out['ws']['graphs_other_pe_form']   # one graph of each form in the workspace: the hit form in use, the full one parked
        assert len(cur) == 1 and len(parked) == 1 and list(cur) == list(parked)
        assert [g[2] for g in cur.values()] == [True] and [g[2] for g in parked.values()] == [False]


def test_hit_frame_against_the_reference_golden():
    """The existing golden tests only ever run first frames, which are misses: the third frame of the seed-0 problem (a hit) against
    tests/golden/micro_s.npz under the bounds of test_gpu_golden.py::test_exact_mode_integer_outputs_equal_the_reference."""
    from test_gpu_golden import index_mismatches, rel
    g = load_golden('micro_s')
    prob = _prob('micro_s', 0)
    eng = _engine(prob, exact=True)
    feat = torch.from_numpy(prob['feat']).to(DEV)
    for want in ('miss', 'build', 'hit'):
        out = eng.run(feat, _props(prob), prob['img_metas'])
        torch.cuda.synchronize()
        assert out['pe_cache'] == want
    R = out['R']
    n_lab, n_idx, n_set, tot = index_mismatches(out, g)
    e_cls = rel(out['cls'][:, :R].reshape(g['cls'].shape), g['cls'])
    e_sc = rel(out['scores'][:tot], g['scores'])
    print(f'[pe_cache] micro_s hit frame: {n_lab}/{tot} ranked labels, {n_idx}/{tot} ranked indices differ; cls rel err {e_cls:.1e}, score rel err {e_sc:.1e}')
    assert e_cls < 3e-6 and e_sc < 1e-5
    assert n_lab == 0 and n_idx in (0, None) and n_set in (0, None)


def test_changing_matrices():
    probs = [_prob('micro_s', s) for s in range(4)]
    engs = [_engine(probs[0]), _engine(probs[0], cache=False)]
    m0 = probs[0]['img_metas']
    m1 = _moved(m0, 0.25)
    seq = [(m0, 'miss'), (m0, 'build'), (m0, 'hit'), (m1, 'miss'), (m0, 'miss'), (m0, 'build'), (m0, 'hit'), (m1, 'miss'), (m1, 'build'), (m1, 'hit')]
    for i, (metas, want) in enumerate(seq):
        p = probs[i % 4]
        got, _ = _frame(engs, torch.from_numpy(p['feat']).to(DEV), _props(p), metas)
        assert got == want, (i, got, want)
    assert engs[0].pe_cache_builds == 3


def test_matrices_that_change_every_frame_never_build():
    probs = [_prob('micro_s', s) for s in range(2)]
    engs = [_engine(probs[0]), _engine(probs[0], cache=False)]
    for i in range(6):
        p = probs[i % 2]
        got, out = _frame(engs, torch.from_numpy(p['feat']).to(DEV), _props(p), _moved(p['img_metas'], 0.01 * (i + 1)))
        assert got == 'miss'
    assert getattr(engs[0], 'pe_cache_builds', 0) == 0 and 'pe_q' not in out['ws']['shared']


def test_new_weights_rebuild_the_table():
    prob = _prob('micro_s', 0)
    sd2 = synthetic.make_head_state(seed=1)
    eng = _engine(prob)
    feat = torch.from_numpy(prob['feat']).to(DEV)
    for want in ('miss', 'build', 'hit'):
        assert eng.run(feat, _props(prob), prob['img_metas'])['pe_cache'] == want
    v0 = eng._weights_version
    eng.load_state(sd2)
    assert eng._weights_version == v0 + 1
    fresh = _engine(prob, sd=sd2, cache=False)
    for want in ('miss', 'build', 'hit'):
        got, _ = _frame([eng, fresh], feat, _props(prob), prob['img_metas'])
        assert got == want
    assert eng.pe_cache_builds == 2


def test_batches():
    pa, pb = _prob('micro_s', 0), _prob('micro_s', 3)
    engs = [_engine(pa), _engine(pa, cache=False)]
    feats = [torch.from_numpy(p['feat']).to(DEV) for p in (pa, pb)]
    props = [_props(pa), _props(pb)]
    m0 = pa['img_metas']
    for want in ('miss', 'build', 'hit'):                         # two samples of one rig: the table of ONE sample serves both
        got, out = _frame(engs, feats, props, [m0, m0], batch=True)
        assert got == want
    sh = out['ws']['shared']
    assert sh['pe_q'].shape[0] == sh['sine_period'] == out['ws']['P'] // 2
    assert int(out['count'][0]) > 0 and int(out['count'][1]) > 0
    builds = engs[0].pe_cache_builds
    for _ in range(3):                                            # two samples of different matrices: uncached
        got, _ = _frame(engs, feats, props, [m0, _moved(m0, 0.5)], batch=True)
        assert got == 'miss'
    assert engs[0].pe_cache_builds == builds


@pytest.mark.parametrize('config', ['fp16_map', 'depth_40'])
def test_other_configurations_hit(config):
    prob = _prob('micro_s', 0)
    kw, sd = {}, None
    if config == 'depth_40':
        sd, kw = synthetic.with_pe_depth_state(synthetic.make_head_state(seed=0), 0, 40), dict(depth_num=40)
    engs = [_engine(prob, sd=sd, **kw), _engine(prob, sd=sd, cache=False, **kw)]
    feat = torch.from_numpy(prob['feat']).to(DEV)
    if config == 'fp16_map':
        feat = feat.half()
    for want in ('miss', 'build', 'hit'):
        got, out = _frame(engs, feat, _props(prob), prob['img_metas'])
        assert got == want
    assert tuple(out['ws']['shared']['pe_q'].shape) == (out['ws']['P'], 256)


@pytest.mark.parametrize('config', ['nofpe', 'micro_t', 'keep_stages'])
def test_routes_that_never_call_the_new_entry(config, monkeypatch):
    from mv2d_amd import ops
    calls = []
    real = ops.pe_gate_x3
    monkeypatch.setattr(ops, 'pe_gate_x3', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    prob = _prob('micro_t' if config == 'micro_t' else 'micro_s', 0)
    kw, sd = {}, None
    if config == 'nofpe':
        sd, kw = synthetic.with_pe_options_state(synthetic.make_head_state(seed=0), False, False), dict(with_fpe=False)
    eng = _engine(prob, sd=sd, **kw)
    feat = torch.from_numpy(prob['feat']).to(DEV)
    for _ in range(3):
        out = eng.run(feat, _props(prob), prob['img_metas'], keep_stages=(config == 'keep_stages'))
        torch.cuda.synchronize()
        assert out['pe_cache'] == 'off' and int(out['count'].item()) > 0
    assert not calls and getattr(eng, 'pe_cache_builds', 0) == 0 and 'pe_q' not in out['ws']['shared']
    if config == 'keep_stages':                                   # ... and the same engine does use it on plain frames
        for want in ('miss', 'build', 'hit'):
            assert eng.run(feat, _props(prob), prob['img_metas'])['pe_cache'] == want
        assert len(calls) == 2
