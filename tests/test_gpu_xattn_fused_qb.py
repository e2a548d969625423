"""The queries per block of the one-launch cross attention (csrc/xattn_fused.hip: 8, or 12 on 12 KB of LDS per query with e4m3 lo rows) only move
WHICH BLOCK AND WAVE compute a query, never how it is computed (-m gpu).  Everything is compared on int32 bit patterns, a NaN only where the other
side has one.

    ops.xattn_fused(qb=...)     qb = 12 against qb = 8 and against the three-kernel path (xattn_qmap, xattn_tile with one wave per query,
                                xattn_ctxmap), with e4m3 lo rows built like tests/test_gpu_xattn_lo.py builds them (f32_to_key16 with lo rows,
                                lo8_encode).  R = 1, 11, 12, 13, 23, 24, 25, 301 -- one query, one short of a block of 12, exactly one, one over,
                                the same around two blocks, a launch of many -- with row lengths cycling through 0, 1, 15, 16, 17, 47, 48, 49, 50,
                                64, 65, 98 keys (the edges of the 16-key tile and of the 49-cell RoI) out of 128 key rows; both empty_nan values,
                                with and without a launch order; outputs in front of guard rows.  The key16-lo and hi-only routes through the same
                                entry stay what the three kernels give, and refuse qb = 12.  One R beyond 12 x the CU count runs deal 1 and 2 in
                                full blocks of 12 (rows of 1 .. 3 keys; the first 24 rows keep the long lengths).
    poisoned inputs             a NaN in one key row, one value row or one query reaches exactly the outputs it reaches at qb = 8.
    HeadEngine.xattn_qb         one micro_s frame through run_batch of 2 samples with the 12-query instance forced through the wrapper's argument:
                                every output is bit for bit that of two single runs on the default."""
import functools

import numpy as np
import pytest
import torch

DEV = 'cuda:0'
SENTINEL = -12345.0
GUARD_ROWS = 64
KEYS = 128
LENGTHS = (0, 1, 15, 16, 17, 47, 48, 49, 50, 64, 65, 98)
QBS = (12,)                       # the instances next to 8 that the library ships


def _bits(a, b):
    """NaN in the same places, the same bits elsewhere"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a.masked_fill(na, 0.0).view(torch.int32), b.masked_fill(nb, 0.0).view(torch.int32))


def _guarded(rows, width=256):
    buf = torch.full(((rows + GUARD_ROWS) * width,), SENTINEL, device=DEV, dtype=torch.float32)
    return buf, buf[:rows * width].view(rows, width)


def _randn(seed, shape, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _tables():
    """what does not depend on R: the key / value tables as key16 hi + lo rows and the lo halves as e4m3 bytes, the packed maps"""
    from mv2d_amd import ops
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    Xk, Xk_lo = ops.f32_to_key16(_randn(8101, (KEYS, 256)).to(DEV), with_lo=True)
    Xv, Xv_lo = ops.f32_to_key16(_randn(8102, (KEYS, 256)).to(DEV), with_lo=True)
    WA, WB = ops.pack_xattn_maps(_randn(8103, (256, 256), 0.06).to(DEV), _randn(8104, (256, 256), 0.06).to(DEV))
    return dict(Xk=Xk, Xv=Xv, lo={'lo8': (ops.lo8_encode(Xk_lo), ops.lo8_encode(Xv_lo)), 'lo16': (Xk_lo, Xv_lo), 'hi': (None, None)}, WA=WA, WB=WB,
                bv=_randn(8105, (256,)).to(DEV))


@functools.lru_cache(maxsize=None)
def _rows(R, short_from=None):
    """queries and a CSR of distinct keys per row: row r lists LENGTHS[(r + 1) % 12] keys (a single row is not empty); from row `short_from` on 1 .. 3 keys"""
    g = np.random.Generator(np.random.PCG64(8200 + R))
    nk = np.array([LENGTHS[(r + 1) % len(LENGTHS)] for r in range(R)])
    if short_from is not None:
        nk[short_from:] = g.integers(1, 4, R - short_from)
    row_ptr = np.concatenate([[0], np.cumsum(nk)]).astype(np.int32)
    col = np.concatenate([g.choice(KEYS, n, replace=False) for n in nk]).astype(np.int32)
    return dict(q=(_randn(8300 + R, (R, 256)) * 0.3).to(DEV), row_ptr=torch.from_numpy(row_ptr).to(DEV), col=torch.from_numpy(col).to(DEV),
                empty=torch.from_numpy(nk == 0).to(DEV), order=torch.randperm(R, generator=torch.Generator().manual_seed(R)).to(torch.int32).to(DEV))


def _three_kernels(t, r, fmt, empty_nan, q=None):
    from mv2d_amd import ops
    Qt = ops.xattn_qmap(r['q'] if q is None else q, t['WA'])
    z = ops.xattn_tile(Qt, t['Xk'], t['Xv'], r['row_ptr'], r['col'], empty_nan=empty_nan, waves=1, Xk_lo=t['lo'][fmt][0], Xv_lo=t['lo'][fmt][1])
    return ops.xattn_ctxmap(z, t['WB'], t['bv'], r['row_ptr'], empty_nan=empty_nan)


def _fused(t, r, fmt, empty_nan, order=None, q=None, **kw):
    from mv2d_amd import ops
    R = r['q'].shape[0]
    buf, out = _guarded(R)
    ops.xattn_fused(r['q'] if q is None else q, t['WA'], t['WB'], t['bv'], t['Xk'], t['Xv'], r['row_ptr'], r['col'], out=out, R=R, empty_nan=empty_nan,
                    Xk_lo=t['lo'][fmt][0], Xv_lo=t['lo'][fmt][1], order=order, **kw)
    torch.cuda.synchronize()
    assert bool((buf[R * 256:] == SENTINEL).all()), (fmt, kw)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('R', [1, 11, 12, 13, 23, 24, 25, 301])
def test_xattn_fused_rows_do_not_depend_on_the_queries_per_block(R):
    t, r = _tables(), _rows(R)
    for empty_nan in (True, False):
        want = _three_kernels(t, r, 'lo8', empty_nan)
        for ordered in (False, True):
            order = r['order'] if ordered else None
            eight = _fused(t, r, 'lo8', empty_nan, order, qb=8)
            assert _bits(eight, want), ('qb 8 against the three kernels', empty_nan, ordered)
            assert _bits(_fused(t, r, 'lo8', empty_nan, order), want), ('the default against the three kernels', empty_nan, ordered)
            for qb in QBS:
                got = _fused(t, r, 'lo8', empty_nan, order, qb=qb)
                assert _bits(got, eight), (qb, 'against qb 8', empty_nan, ordered)
                assert _bits(got, want), (qb, 'against the three kernels', empty_nan, ordered)
        rows_nan = torch.isnan(eight).all(1)
        assert torch.equal(rows_nan, r['empty'] if empty_nan else torch.zeros_like(r['empty']))
        # the other two routes through the same entry: what they were
        for fmt in ('lo16', 'hi'):
            w = _three_kernels(t, r, fmt, empty_nan)
            assert _bits(_fused(t, r, fmt, empty_nan), w) and _bits(_fused(t, r, fmt, empty_nan, r['order'], qb=8), w), (fmt, empty_nan)
    for fmt in ('lo16', 'hi'):
        with pytest.raises(Exception):
            _fused(t, r, fmt, True, qb=12)
    with pytest.raises(Exception):
        _fused(t, r, 'lo8', True, qb=16)


@pytest.mark.gpu
def test_xattn_fused_full_blocks_of_twelve_under_both_deals():
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    R = 12 * n_cu + 37                                            # more blocks of 12 than CUs: the dealing branch, blocks of 11 .. 12 queries
    t, r = _tables(), _rows(R, short_from=24)
    for empty_nan in (True, False):
        want = _three_kernels(t, r, 'lo8', empty_nan)
        for ordered in (False, True):
            order = r['order'] if ordered else None
            assert _bits(_fused(t, r, 'lo8', empty_nan, order), want), ('the default', empty_nan, ordered)
            for qb in (8,) + QBS:
                for deal in (1, 2):
                    assert _bits(_fused(t, r, 'lo8', empty_nan, order, qb=qb, deal=deal), want), (qb, deal, empty_nan, ordered)


@pytest.mark.gpu
@pytest.mark.parametrize('what', ['key', 'value', 'query'])
def test_a_poisoned_input_reaches_the_same_outputs(what):
    """One NaN in a key row, a value row or a query: the rows that read it (and only those) differ from the clean run, the same rows and the same bits
    at every number of queries per block."""
    R = 25
    t, r = dict(_tables()), _rows(R)
    q = r['q']
    nan16 = torch.tensor(float('nan'), dtype=t['Xk'].dtype)
    if what == 'query':
        q = q.clone()
        q[13, 77] = float('nan')
        hit = torch.zeros(R, dtype=torch.bool)
        hit[13] = True
    else:
        name = 'Xk' if what == 'key' else 'Xv'
        t[name] = t[name].clone()
        t[name].view(-1)[5 * 256 + 130] = nan16                  # key row 5
        rp, col = r['row_ptr'].cpu().numpy(), r['col'].cpu().numpy()
        hit = torch.tensor([5 in col[rp[i]:rp[i + 1]] for i in range(R)])
    assert 0 < int(hit.sum()) < R
    clean = _fused(_tables(), r, 'lo8', False, qb=8)
    eight = _fused(t, r, 'lo8', False, q=q, qb=8)
    assert _bits(eight, _three_kernels(t, r, 'lo8', False, q=q))
    assert torch.equal(torch.isnan(eight).any(1).cpu(), hit), 'the NaN is visible in every row that reads it and in no other'
    assert _bits(eight[~hit.to(DEV)], clean[~hit.to(DEV)])
    for qb in QBS:
        for order in (None, r['order']):
            assert _bits(_fused(t, r, 'lo8', False, order, q=q, qb=qb), eight), (what, qb)


@pytest.mark.gpu
def test_engine_batch_on_twelve_queries_per_block_equals_single_runs(monkeypatch):
    """micro_s: run_batch of 2 samples with the 12-query instance forced through the wrapper's argument (HeadEngine.xattn_qb) against two single runs
    on the default: every output tensor bit for bit, and the wrapper receives the argument in every layer."""
    from mv2d_amd import ops, synthetic
    from mv2d_amd.engine import HeadEngine
    dev = torch.device(DEV)
    sd = synthetic.make_head_state(seed=0)
    probs = [synthetic.make_problem('micro_s', seed=s) for s in (0, 10)]
    feats = [torch.from_numpy(p['feat']).to(dev) for p in probs]
    props = [[torch.from_numpy(x) for x in p['proposals']] for p in probs]
    metas = [p['img_metas'] for p in probs]
    seen, real = [], ops.xattn_fused

    def spy(*a, **kw):
        seen.append(kw.get('qb'))
        return real(*a, **kw)
    monkeypatch.setattr(ops, 'xattn_fused', spy)

    single = HeadEngine(sd, 'S', dev, num_views=probs[0]['views_per_frame'])
    assert single.xattn_qb == 0
    refs = [{k: v.clone() for k, v in single.run(feats[b], props[b], metas[b]).items() if isinstance(v, torch.Tensor)} for b in range(2)]       # (a run's tensors are workspace views)
    res_single = [[x.clone() for x in single.results(single.run(feats[b], props[b], metas[b]))] for b in range(2)]
    assert seen and set(seen) == {None}
    del seen[:]

    eng = HeadEngine(sd, 'S', dev, num_views=probs[0]['views_per_frame'])

    def frame(use_graph):
        out = eng.run_batch(feats, props, metas, use_graph=use_graph)
        torch.cuda.synchronize()
        grp = out['grp_start'].tolist()
        return ([{k: out[k][:, grp[b]:grp[b + 1]].clone() for k in ('cls', 'reg')} for b in range(2)],
                [[x.clone() for x in rb] for rb in eng.results_batch(out)])

    for qb in (0, 12):
        eng.xattn_qb = qb
        del seen[:]
        for use_graph in (False, True):
            rows, res = frame(use_graph)
            for b in range(2):
                for k in ('cls', 'reg'):
                    assert _bits(rows[b][k], refs[b][k]), (qb, use_graph, b, k)
                for a, w in zip(res[b], res_single[b]):
                    same = _bits(a, w) if a.dtype == torch.float32 else torch.equal(a, w)
                    assert same, (qb, use_graph, b)
        assert seen and set(seen) == {qb or None}
    with pytest.raises(ValueError, match='xattn_qb'):
        eng.xattn_qb = 9
        eng.run_batch(feats, props, metas)
