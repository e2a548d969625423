"""The gate-only PE kernel on a cached frustum MLP (pe_x3_gate_kernel, mv2d_pe_gate_x3; csrc/pe_x3_gate.hip): pe = tab[pos] + Q[pos] * gate(feature row)
with Q = what the gate-less entry writes on a one-row zero table, BIT FOR BIT the pe of the full kernel (ops.pe_fused_x3) on the frustum rows Q was
built from -- at the tile edges, through a gather that wraps the period, with a device-side row count, for the three map formats and two depths;
the NaN / Inf rule; the refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PERIOD, NPOS = 70, 210                      # a map of 3 x 70 positions over a rig of period 70: row_index % PERIOD wraps
SENTINEL = -7.5


def rnd(shape, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def _kp(D):
    return 32 * ((3 * D + 31) // 32)


_CASE = {}


def _case(D):
    """Weights, biases, table, the frustum rows of the PERIOD positions of one sample, the feature map and Q for one depth: built once, shared by the
    tests, never written."""
    if D not in _CASE:
        from mv2d_amd import ops
        W = dict(w1a=rnd((1024, 3 * D), 193 + D, 0.08 * (192.0 / (3 * D)) ** 0.5), w1b=rnd((256, 1024), 194, 0.04), wr=rnd((256, 256), 197, 0.07),
                 we=rnd((256, 256), 198, 0.07))
        wx = {k: ops.pack_x3(ops.pad_pe_w1a(v.to(DEV), D) if k == 'w1a' else v.to(DEV)) for k, v in W.items()}
        wx.update({k: rnd((n,), 199 + i).to(DEV) for i, (k, n) in enumerate(dict(b1a=1024, b1b=256, br=256, be=256).items())})
        tab = rnd((PERIOD, 256), 231).to(DEV)
        A1 = torch.zeros((PERIOD, _kp(D)), device=DEV)
        A1[:, :3 * D] = (rnd((PERIOD, 3 * D), 190 + D) * 3.0).to(DEV)
        Xmap = rnd((NPOS, 256), 192).to(DEV)
        Q = torch.empty((PERIOD, 256), device=DEV)
        ops.pe_fused_x3(A1, None, None, wx, torch.zeros((1, 256), device=DEV), 1, pe=Q, M=PERIOD, Kp=_kp(D), gate=False)
        _CASE[D] = dict(wx=wx, tab=tab, A1=A1, Xmap=Xmap, Q=Q)
    return _CASE[D]


def _rows(M, seed=6):
    """M distinct map positions in a permuted order (rows of every third of the map: the period wraps)"""
    return torch.randperm(NPOS, generator=torch.Generator().manual_seed(seed))[:M].to(torch.int32).to(DEV)


def _both(c, D, M, ri, md=None, at_index=False, Xmap=None, Q=None, n_out=None):
    """(full kernel, gate-only kernel) on the same rows into sentinel-filled buffers"""
    from mv2d_amd import ops
    Xmap = c['Xmap'] if Xmap is None else Xmap
    pos = (ri.long() if ri is not None else torch.arange(M, device=DEV)) % PERIOD
    n_out = (NPOS if at_index else M) if n_out is None else n_out
    ref = torch.full((n_out, 256), SENTINEL, device=DEV)
    got = torch.full((n_out, 256), SENTINEL, device=DEV)
    ops.pe_fused_x3(c['A1'][pos].contiguous(), Xmap, md, c['wx'], c['tab'], PERIOD, pe=ref, M=M, row_index=ri, Kp=_kp(D), pe_at_index=at_index)
    ops.pe_gate_x3(c['Q'] if Q is None else Q, Xmap, md, c['wx'], c['tab'], PERIOD, got, M, row_index=ri, pe_at_index=at_index)
    return ref, got


@pytest.mark.parametrize('at_index', [False, True])
@pytest.mark.parametrize('M', [1, 63, 64, 65, 200])
def test_gate_only_equals_the_full_kernel_bitwise(M, at_index):
    """One row, the tile edge from both sides, several tiles with a ragged tail; permuted row_index over 3 periods; pe rows in launch order and at
    their map positions.  Rows nobody addresses keep the sentinel."""
    c = _case(64)
    ri = _rows(M)
    ref, got = _both(c, 64, M, ri, at_index=at_index)
    assert torch.equal(got, ref)
    written = ri.long() if at_index else torch.arange(M, device=DEV)
    rest = torch.ones(ref.shape[0], dtype=torch.bool, device=DEV)
    rest[written] = False
    assert bool((got[written] != SENTINEL).any(1).all()) and bool((got[rest] == SENTINEL).all())
    assert int(rest.sum()) == ref.shape[0] - M


def test_gate_only_without_row_index():
    c = _case(64)
    ref, got = _both(c, 64, 65, None)
    assert torch.equal(got, ref) and bool((got != SENTINEL).any(1).all())


@pytest.mark.parametrize('at_index', [False, True])
def test_device_side_row_count(at_index):
    """m_dev = 130 of M = 200 launched rows: rows past 130 are untouched."""
    c = _case(64)
    ri = _rows(200)
    md = torch.tensor([130], dtype=torch.int32, device=DEV)
    ref, got = _both(c, 64, 200, ri, md=md, at_index=at_index)
    assert torch.equal(got, ref)
    past = ri[130:].long() if at_index else torch.arange(130, 200, device=DEV)
    done = ri[:130].long() if at_index else torch.arange(130, device=DEV)
    assert bool((got[past] == SENTINEL).all()) and bool((got[done] != SENTINEL).any(1).all())
    # a count above M is clamped to M; a count of 0 writes nothing
    big = torch.tensor([1000], dtype=torch.int32, device=DEV)
    ref2, got2 = _both(c, 64, 65, ri[:65].contiguous(), md=big)
    assert torch.equal(got2, ref2) and bool((got2 != SENTINEL).any(1).all())
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    _, got0 = _both(c, 64, 65, ri[:65].contiguous(), md=zero)
    assert bool((got0 == SENTINEL).all())


@pytest.mark.parametrize('D', [64, 8])
@pytest.mark.parametrize('map_dtype', [torch.float32, torch.float16, torch.bfloat16])
def test_map_formats_and_depths(map_dtype, D):
    """The three map formats; Q built at Kp = 192 (64 bins) and Kp = 32 (8 bins): the gate kernel is the same instance for both depths.  A 16-bit map
    is widened in the kernel: also bitwise the fp32 call on x.float()."""
    from mv2d_amd import ops
    c = _case(D)
    assert tuple(c['A1'].shape) == (PERIOD, 192 if D == 64 else 32)
    ri = _rows(200)
    md = torch.tensor([187], dtype=torch.int32, device=DEV)
    x = c['Xmap'].to(map_dtype)
    ref, got = _both(c, D, 200, ri, md=md, at_index=True, Xmap=x)
    assert torch.equal(got, ref) and float(got[ri[:187].long()].abs().sum()) > 0
    if map_dtype != torch.float32:
        wide = torch.full_like(got, SENTINEL)
        ops.pe_gate_x3(c['Q'], x.float(), md, c['wx'], c['tab'], PERIOD, wide, 200, row_index=ri, pe_at_index=True, map_fmt=0)
        assert torch.equal(wide, got)
        with pytest.raises(Exception, match='map_fmt'):
            ops.pe_gate_x3(c['Q'], x, md, c['wx'], c['tab'], PERIOD, wide, 200, row_index=ri, map_fmt=0)


def test_nan_and_inf_stay_in_their_rows():
    """One NaN in a feature row makes exactly that pe row NaN (the rule round 6 set for the attention kernel: a poisoned row shows, and only it); an
    Inf in one Q row reaches the rows at that position only."""
    c = _case(64)
    M = 200
    ri = _rows(M)
    x = c['Xmap'].clone()
    bad = int(ri[77])
    x[bad, 131] = float('nan')
    ref, got = _both(c, 64, M, ri, Xmap=x)
    nan_rows = torch.isnan(got).any(1)
    assert bool(torch.isnan(got[77]).all()) and int(nan_rows.sum()) == 1
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    keep = ~nan_rows
    assert torch.equal(got[keep], ref[keep])
    q = c['Q'].clone()
    qpos = int(ri[5]) % PERIOD
    q[qpos, 5] = float('inf')
    _, got = _both(c, 64, M, ri, Q=q)
    hit = (ri.long() % PERIOD) == qpos
    assert 1 <= int(hit.sum()) <= 3
    assert bool(torch.isinf(got[hit][:, 5]).all()) and int((~torch.isfinite(got)).sum()) == int(hit.sum())
    clean, _ = _both(c, 64, M, ri)
    mask = torch.ones_like(got, dtype=torch.bool)
    mask[hit, 5] = False
    assert torch.equal(got[mask], clean[mask])


def test_refusals_name_the_entry():
    from mv2d_amd import _lib, ops
    c = _case(64)
    M = 8
    ri = _rows(M)
    pe = torch.zeros((M, 256), device=DEV)
    k16 = ops.key16_dtype()
    pair = (torch.zeros((M, 256), device=DEV, dtype=k16), torch.zeros((M, 256), device=DEV, dtype=k16))
    args = (c['Q'], c['Xmap'], None, c['wx'], c['tab'])
    for kw in (dict(Xk=pair, Xv=pair), dict(Xk=pair), dict(Xv=pair)):
        with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_gate_x3.*key / value row'):
            ops.pe_gate_x3(*args, PERIOD, pe, M, row_index=ri, **kw)
    with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_gate_x3.*pe.*expected torch.float32'):
        ops.pe_gate_x3(*args, PERIOD, pe.half(), M, row_index=ri)
    with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_gate_x3.*Q.*expected torch.float32'):
        ops.pe_gate_x3(c['Q'].double(), *args[1:], PERIOD, pe, M, row_index=ri)
    with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_gate_x3.*row_index.*expected torch.int32'):
        ops.pe_gate_x3(*args, PERIOD, pe, M, row_index=ri.long())
    with pytest.raises(ValueError, match='feature map of dtype'):
        ops.pe_gate_x3(c['Q'], c['Xmap'].double(), None, c['wx'], c['tab'], PERIOD, pe, M, row_index=ri)
    for period in (0, -3):
        with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_gate_x3.*tab_period > 0'):
            ops.pe_gate_x3(*args, period, pe, M, row_index=ri)
    with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_gate_x3.*tab_period = 64'):          # a Q of another period than stated
        ops.pe_gate_x3(*args, 64, pe, M, row_index=ri)
    with pytest.raises(_lib.Mv2dHipError, match='mv2d_pe_gate_x3.*pe_at_index needs row_index'):
        _lib_call_at_index_without_rows(c, pe, M)
    torch.cuda.synchronize()
    assert not pe.any()


def _lib_call_at_index_without_rows(c, pe, M):
    from mv2d_amd import _lib, ops
    p, wx = (lambda t: t.data_ptr()), c['wx']
    rc = _lib.load().mv2d_pe_gate_x3(p(c['Q']), p(c['Xmap']), None, None, M, p(wx['wr'][0]), p(wx['wr'][1]), p(wx['br']), p(wx['we'][0]), p(wx['we'][1]),
                                     p(wx['be']), p(c['tab']), PERIOD, p(pe), None, None, None, None, 1, 0, None)
    ops.check(rc, 'mv2d_pe_gate_x3')
