"""The cases of tests/rowblock_cases.py can carry the bounds of tests/test_gpu_rowblock_edges.py (CPU only, no library).  The yardstick of an
output is the largest per-row error (max |error| over max |reference| of the row) of its plain fp32 evaluation against fp64.

Rows (operands of rowblock_cases.operands(), all 545 rows): the format model -- every product a_hi w_hi + a_lo w_hi + a_hi w_lo on fp16 pairs --
stays within FORMAT_ROOM = 4 yardsticks on every row of every output (measured: x 0.67, q 0.34, Qt 0.97, z-form x 0.69, qkv 0.40 .. 0.48; y, xq
and outs contain no product and are the fp64 reference itself).  Either lo product lost moves EVERY row of every output that contains a product
(x, q, Qt, the z-form x, qkv at every slab count) by at least 3 x K_ROWS yardsticks; measured smallest row, a_lo w_hi lost / a_hi w_lo lost:
x 95 / 82, q 97 / 89, Qt 265 / 266, z-form x 98 / 96, qkv 98 .. 124 / 105 .. 133 (worst rows 265 .. 723).  Qt and qkv needed no change of the
operands.  y, xq and outs cannot move: no product precedes them; a lost guard or a wrong row there is what the GPU test's identities with
ops.row_ln and between the block shapes are for.

Self-attention (one yardstick per case, over all rows): on 'plain' the two key mutants move every row of every sample of two or more keys by at
least 4 x K_SA yardsticks (measured smallest row 9784, in the 255-key sample); on 'sharp' the worst row of every such sample (measured
89 574 and more; single rows of the long samples see their last key with a probability near 0 and move by as little as 12)."""
import pytest
import torch

import rowblock_cases as rc

F64, F32 = torch.float64, torch.float32
FORMAT_ROOM = 4.0
MUTANTS = ('a_lo', 'w_lo')


def _ratios(got, ref, f32, rows=None):
    """(per-row errors of `got` in yardsticks, the yardstick) over the rows `rows`"""
    yard = rc.yardstick(f32, ref, rows)
    assert 0.0 < yard < 1e-5 and yard == yard, yard                   # finite, positive, fp32-class
    e = rc.row_errors(got, ref)
    return (e if rows is None else e[rows]) / yard, yard


def _hold_format_and_mutants(name, ref, f32, model, mutants, rows=None):
    r, yard = _ratios(model, ref, f32, rows)
    print(f'{name}: yardstick {yard:.3e}, format model {float(r.max()):.2f}')
    assert float(r.max()) <= FORMAT_ROOM, (name, float(r.max()))
    for drop, res in mutants.items():
        r, _ = _ratios(res, ref, f32, rows)
        print(f'{name}: {drop} product lost, smallest row {float(r.min()):.1f}, largest {float(r.max()):.1f} yardsticks')
        assert float(r.min()) >= 3.0 * rc.K_ROWS, (name, drop, float(r.min()))


def test_bounds_respect_their_caps():
    assert rc.K_ROWS <= 16.0 and rc.K_SA <= 64.0 and rc.K_SA == max(rc.K_SA_X3_PLAIN, rc.K_SA_X3_SHARP, rc.K_SA_F32)


def test_csr_has_exactly_the_named_empty_rows():
    o = rc.operands()
    nk = (o.row_ptr[1:] - o.row_ptr[:-1]).tolist()
    assert o.row_ptr.dtype == torch.int32 and o.row_ptr.numel() == rc.M_ALL + 1 and int(o.row_ptr[0]) == 0
    assert tuple(m for m, n in enumerate(nk) if n == 0) == rc.EMPTY_ROWS == (0, 15, 16, 511, 512, 527, 528, 544)
    assert min(nk) == 0 and all(n >= 1 for m, n in enumerate(nk) if m not in rc.EMPTY_ROWS)
    assert tuple(o.empty.nonzero().flatten().tolist()) == rc.EMPTY_ROWS
    assert rc.ROW_COUNTS == (1, 16, 17, 512, 513, 528, 529, 545) and rc.M_ALL == 545 and rc.QSCALE == 1.0 / 32.0 ** 0.5


def test_attn_chain_format_model_and_lo_mutants():
    ref, f32, model = rc.attn_refs(F64), rc.attn_refs(F32), rc.attn_chain(prod=rc.Q16Model())
    mut = {d: rc.attn_chain(prod=rc.Q16Model(d)) for d in MUTANTS}
    for k in ('x', 'q', 'Qt'):
        _hold_format_and_mutants(k, getattr(ref, k), getattr(f32, k), getattr(model, k), {d: getattr(m, k) for d, m in mut.items()})


@pytest.mark.parametrize('empty_nan', [True, False])
def test_zmap_chain_format_model_and_lo_mutants(empty_nan):
    o = rc.operands()
    ref, f32 = rc.zmap_refs(F64, empty_nan), rc.zmap_refs(F32, empty_nan)
    model = rc.zmap_chain(prod=rc.Q16Model(), empty_nan=empty_nan)
    mut = {d: rc.zmap_chain(prod=rc.Q16Model(d), empty_nan=empty_nan) for d in MUTANTS}
    _hold_format_and_mutants(f'z-form x (empty_nan={empty_nan})', ref.x, f32.x, model.x, {d: m.x for d, m in mut.items()}, rows=~o.empty)
    for res in (ref, f32, model, *mut.values()):                      # the empty rows: all-NaN, or LN(bo + resid) -- not LN(bv Wo^T + ...)
        if empty_nan:
            assert bool(torch.isnan(res.x[o.empty]).all()) and not bool(torch.isnan(res.x[~o.empty]).any())
            assert bool(torch.isnan(res.ctx[o.empty]).all())
        else:
            assert float(res.ctx[o.empty].abs().max()) == 0.0
    if not empty_nan:
        t = lambda a: a.double()
        want = torch.nn.functional.layer_norm(t(o.bo) + t(o.resid), (256,), t(o.lw), t(o.lb), rc.EPS)
        assert float(rc.row_errors(ref.x, want)[o.empty].max()) <= 2.0 ** -40
        assert float(rc.row_errors(model.x, want)[o.empty].max()) == 0.0          # 0 splits into (0, 0): the products vanish exactly


@pytest.mark.parametrize('n_parts', rc.PARTS_COUNTS)
def test_tail_chain_format_model_and_lo_mutants(n_parts):
    ref, f32 = rc.tail_refs(F64, n_parts), rc.tail_refs(F32, n_parts)
    model = rc.tail_chain(prod=rc.Q16Model(), n_parts=n_parts)
    mut = {d: rc.tail_chain(prod=rc.Q16Model(d), n_parts=n_parts) for d in MUTANTS}
    _hold_format_and_mutants(f'qkv n_parts={n_parts}', ref.qkv, f32.qkv, model.qkv, {d: m.qkv for d, m in mut.items()})
    for k in ('y', 'xq', 'outs'):                                      # no product in front of them: the model is the reference
        r, yard = _ratios(getattr(model, k), getattr(ref, k), getattr(f32, k))
        print(f'{k} n_parts={n_parts}: yardstick {yard:.3e}')
        assert float(r.max()) == 0.0


def test_references_of_a_row_slice_are_the_slice_of_the_references():
    """Rows are independent: the identities of the GPU test (first M rows, [0:512] + [512:M]) rest on it.  fp64 BLAS may block another row
    count differently, so equal means to 2^-40 of a row's maximum."""
    tol = 2.0 ** -40
    same = lambda a, b: float(rc.row_errors(a, b).nan_to_num(0.0).max()) <= tol and torch.equal(torch.isnan(a), torch.isnan(b))
    a, t = rc.attn_refs(F64), rc.tail_refs(F64, 23)
    for sl in [slice(0, M) for M in rc.ROW_COUNTS] + [slice(512, M) for M in rc.ROW_COUNTS if M > 512]:
        s = rc.attn_chain(rows=sl)
        assert same(s.x, a.x[sl]) and same(s.q, a.q[sl]) and same(s.Qt, a.Qt[sl]), sl
        for en in (True, False):
            assert same(rc.zmap_chain(rows=sl, empty_nan=en).x, rc.zmap_refs(F64, en).x[sl]), sl
        s = rc.tail_chain(rows=sl, n_parts=23)
        assert same(s.y, t.y[sl]) and same(s.xq, t.xq[sl]) and same(s.outs, t.outs[sl]) and same(s.qkv, t.qkv[sl]), sl
    assert rc.attn_chain(rows=17).x.shape == (17, 256) and rc.tail_chain(rows=slice(512, 529)).qkv.shape == (17, 768)


def test_self_attention_batch_layout():
    case = rc.sa_case('plain')
    assert case.sizes == (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257) and case.R == 1491 and rc.SA_PAD == 40
    assert case.qkv.shape == (1491 + 40, 768) and case.grp_start.dtype == torch.int32
    assert case.grp_start.tolist() == [sum(case.sizes[:i]) for i in range(len(case.sizes) + 1)]
    sharp = rc.sa_case('sharp')
    assert torch.equal(sharp.qkv[:, :256], case.qkv[:, :256] * 3.0) and torch.equal(sharp.qkv[:, 256:], case.qkv[:, 256:])
    ref = rc.sa_refs('plain')[1]
    assert torch.equal(ref[:1], case.qkv[:1, 512:].double())          # the one-key sample: its value row


@pytest.mark.parametrize('kind', ['plain', 'sharp'])
@pytest.mark.parametrize('mutant', ['drop_last', 'dup_last'])
def test_self_attention_key_mutants_show(kind, mutant):
    case, ref, yard = rc.sa_refs(kind)
    assert 0.0 < yard < 1e-5
    r = rc.row_errors(rc.sa_attend(case, mutant=mutant), ref) / yard
    assert float(r[0]) == 0.0                                         # one key: nothing to drop or to count twice
    for o, n in zip(case.starts, case.sizes):
        if n >= 2:
            lo, hi = float(r[o:o + n].min()), float(r[o:o + n].max())
            print(f'self-attention {kind} {mutant}, sample of {n}: smallest row {lo:.0f}, largest {hi:.0f} yardsticks ({yard:.3e})')
            assert (lo if kind == 'plain' else hi) >= 4.0 * rc.K_SA, (kind, mutant, n, lo, hi)
