"""The one-launch tail of the query generator (ops.qg_tail_x3, csrc/qg_tail.hip) against the four launches it replaces
(ops.linear_x3 x 3 + ops.query_embed_fused_x3) on the same random weights and inputs: all five outputs BIT FOR BIT (int32 views), at the
edges of a 16-row MFMA tile and of a 32-row block; and the engine with the switch on / off (-m gpu)."""
import sys

import pytest
import torch

from mv2d_amd import synthetic

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 31, 32, 33, 65, 97)
RMAX = 128                      # buffer rows: rows >= R carry a sentinel that must survive
SENTINEL = -12345.0
OUTS = (('center', 3), ('xyz', 3), ('ref', 3), ('posemb', 384), ('qpos', 256))
PC_RANGE = (-61.2, -61.2, -10.0, 61.2, 61.2, 10.0)


def _dev():
    return torch.device('cuda:0')


_cache = {}


def weights():
    """Random weights of the shipped dimensions, packed once and shared (read-only) by every case."""
    if 'w' in _cache:
        return _cache['w']
    from mv2d_amd import ops
    g = torch.Generator().manual_seed(7)
    d = _dev()
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(d)
    w = dict(fc=rn(1024, 256, scale=256 ** -0.5), fc_b=rn(1024, scale=0.1), e0=rn(512, 1056, scale=1056 ** -0.5), e0_b=rn(512, scale=0.1),
             e2=rn(256, 512, scale=512 ** -0.5), e2_b=rn(256, scale=0.1), c_w=rn(3, 256, scale=256 ** -0.5), c_b=rn(3, scale=0.5),
             q0=rn(256, 384, scale=384 ** -0.5), q0_b=rn(256, scale=0.1), q2=rn(256, 256, scale=256 ** -0.5), q2_b=rn(256, scale=0.1))
    for k in ('fc', 'e0', 'e2', 'q0', 'q2'):
        w[k + '_x'] = ops.pack_x3(w[k])
    w['dim_t'] = (10000.0 ** (2 * (torch.arange(128) // 2).float() / 128)).to(d)
    w['pc'] = torch.tensor(PC_RANGE, dtype=torch.float32)
    _cache['w'] = w
    return w


def inputs(seed, x2_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    d = _dev()
    x2 = (torch.randn(RMAX, 256, generator=g).abs() * x2_scale).to(d)            # (the conv's output is post-ReLU)
    enc = torch.full((RMAX, 1056), SENTINEL, device=d)
    enc[:, 1024:] = torch.randn(RMAX, 32, generator=g).to(d)
    minv = torch.randn(RMAX, 16, generator=g).to(d)
    return x2, enc, minv


def fresh_outs():
    return {k: torch.full((RMAX, n), SENTINEL, device=_dev()) for k, n in OUTS}


def chain(w, x2, enc, minv, R, fc_b=None, e0_b=None):
    """The four launches.  Returns the outputs and the hidden layers."""
    from mv2d_amd import ops
    enc = enc.clone()
    enc1, enc2 = torch.zeros((RMAX, 512), device=x2.device), torch.zeros((RMAX, 256), device=x2.device)
    o = fresh_outs()
    ops.linear_x3(x2, w['fc_x'], w['fc_b'] if fc_b is None else fc_b, N=1024, K=256, act=1, clamp=5e3, out=enc, ldc=1056, M=R)
    ops.linear_x3(enc, w['e0_x'], w['e0_b'] if e0_b is None else e0_b, N=512, K=1056, act=1, out=enc1, M=R)
    ops.linear_x3(enc1, w['e2_x'], w['e2_b'], N=256, K=512, act=1, out=enc2, M=R)
    ops.query_embed_fused_x3(enc2, w['c_w'], w['c_b'], minv, w['dim_t'], w['pc'], w['q0_x'], w['q0_b'], w['q2_x'], w['q2_b'], o['center'], o['xyz'],
                             o['ref'], o['posemb'], o['qpos'], R=R)
    return o, dict(enc=enc, enc1=enc1, enc2=enc2)


def fused(w, x2, enc, minv, R, fc_b=None, e0_b=None):
    from mv2d_amd import ops
    o = fresh_outs()
    enc = enc.clone()
    ops.qg_tail_x3(x2, enc, w['fc_x'], w['fc_b'] if fc_b is None else fc_b, w['e0_x'], w['e0_b'] if e0_b is None else e0_b, w['e2_x'], w['e2_b'],
                   w['c_w'], w['c_b'], minv, w['dim_t'], w['pc'], w['q0_x'], w['q0_b'], w['q2_x'], w['q2_b'], o['center'], o['xyz'], o['ref'],
                   o['posemb'], o['qpos'], R=R)
    return o, enc


def assert_bitwise(got, want, R, what):
    for k, _ in OUTS:
        a, b = got[k][:R].contiguous().view(torch.int32), want[k][:R].contiguous().view(torch.int32)
        n = int((a != b).sum())
        assert n == 0, f'{what}: {k}: {n} of {a.numel()} elements differ'
        assert bool((got[k][R:] == SENTINEL).all()), f'{what}: {k}: rows >= R were written'


@pytest.mark.parametrize('R', ROWS)
def test_qg_tail_bitwise_equals_the_four_launches(R):
    w = weights()
    x2, enc, minv = inputs(100 + R)
    want, _ = chain(w, x2, enc, minv, R)
    got, enc_after = fused(w, x2, enc, minv, R)
    assert_bitwise(got, want, R, f'R={R}')
    assert torch.equal(enc_after, enc), 'the fused launch must not write enc'
    assert bool(torch.isfinite(want['qpos'][:R]).all()) and float(want['qpos'][:R].abs().max()) > 0


def test_qg_tail_large_launch(monkeypatch):
    """2049 rows: 65 compute blocks (a ragged last one) -- the size from which the launch adds its L2-warming blocks."""
    monkeypatch.setattr(sys.modules[__name__], 'RMAX', 2080)
    w, R = weights(), 2049
    x2, enc, minv = inputs(9)
    want, _ = chain(w, x2, enc, minv, R)
    got, _ = fused(w, x2, enc, minv, R)
    assert_bitwise(got, want, R, 'R=2049')


def test_qg_tail_clamp_bites():
    """x2 scaled until fc outputs exceed 5e3: the fused launch must clamp exactly where linear_x3 does."""
    from mv2d_amd import ops
    w, R = weights(), 33
    x2, enc, minv = inputs(5, x2_scale=2000.0)
    want, hid = chain(w, x2, enc, minv, R)
    raw = ops.linear_x3(x2, w['fc_x'], w['fc_b'], N=1024, K=256, act=1, clamp=0.0, M=R)          # the same layer without the clamp
    over = raw[:R] > 5e3
    assert int(over.sum()) > 0, 'the case must drive some fc outputs beyond the clamp'
    assert bool((hid['enc'][:R, :1024][over] == 5e3).all()) and float(hid['enc'][:R, :1024].max()) == 5e3
    got, _ = fused(w, x2, enc, minv, R)
    assert_bitwise(got, want, R, 'clamp')


def test_qg_tail_zero_enc1_tile():
    """Negative extra_enc.0 biases: enc1 is zero after its ReLU for whole 16-row tiles."""
    w, R = weights(), 33
    x2, enc, minv = inputs(6)
    e0_b = torch.full((512,), -1e4, device=_dev())
    want, hid = chain(w, x2, enc, minv, R, e0_b=e0_b)
    assert float(hid['enc1'][:32].abs().max()) == 0.0, 'the case must zero the first two row tiles of enc1'
    got, _ = fused(w, x2, enc, minv, R, e0_b=e0_b)
    assert_bitwise(got, want, R, 'zero enc1')


# ---------------------------------------------------------------------------------------------------------------- engine level
NAME = 'micro_s'                # the smallest S workload of synthetic.WORKLOADS
KEYS = ('cls', 'reg', 'boxes', 'scores', 'labels', 'bbox_index', 'count')


def _two_samples():
    """two samples with different RoI counts: the launch runs on the bucket size, so padding rows exist"""
    out = []
    for i, drop in enumerate((0, 2)):
        prob = synthetic.make_problem(NAME, seed=10 * i)
        props = [torch.from_numpy(p[:max(1, p.shape[0] - drop - j)]) for j, p in enumerate(prob['proposals'])]
        out.append((torch.from_numpy(prob['feat']), props, prob['img_metas'], prob['views_per_frame']))
    return out


def _engine(fuse):
    from mv2d_amd.engine import HeadEngine
    s = _two_samples()
    eng = HeadEngine(synthetic.make_head_state(seed=0), 'S', _dev(), num_views=s[0][3])
    eng.fuse_qg_tail = fuse
    return eng, [x[0].to(_dev()) for x in s], [x[1] for x in s], [x[2] for x in s]


def _frame(eng, feats, props, metas, **kw):
    out = eng.run_batch(feats, props, metas, **kw)
    torch.cuda.synchronize()
    return out, {k: out[k].clone() for k in KEYS}


@pytest.mark.parametrize('use_graph', [False, True])
def test_engine_fused_tail_equals_four_launches(use_graph):
    res = {}
    for fuse in (True, False):
        eng, feats, props, metas = _engine(fuse)
        out, res[fuse] = _frame(eng, feats, props, metas, use_graph=use_graph)
        assert out['ws']['route'].qg_tail_fused == fuse
        assert len({sum(p.shape[0] for p in pl) for pl in props}) == 2 and out['ws']['qpos'].shape[0] > out['R'], 'no padding rows in this launch'
    for k in KEYS:
        assert torch.equal(res[True][k], res[False][k]), k
    assert bool(torch.isfinite(res[True]['cls']).all())


def test_engine_keep_stages_still_fills_enc():
    eng, feats, props, metas = _engine(True)
    out, _ = _frame(eng, feats, props, metas)
    qpos = out['ws']['qpos'][:out['R']].clone()
    st_out, _ = _frame(eng, feats, props, metas, keep_stages=True)
    assert not st_out['ws']['route'].qg_tail_fused
    enc = st_out['stages']['enc']
    assert enc.shape == (out['R'], 1056) and float(enc[:, :1024].abs().max()) > 0 and int((enc[:, :1024] != 0).any(1).sum()) == out['R']
    assert torch.equal(st_out['stages']['qpos'], qpos)
