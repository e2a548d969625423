"""The cases of tests/train_cases.py can carry the bounds of tests/test_gpu_train_edges.py (CPU only, no library).  The yardstick of an output is
the largest row error (train_cases.row_err) of its plain fp32 evaluation against fp64 over the cases of its family; for the dense block, whose
products run on bf16 hi + lo pairs, that of the format model Bf16x3 per operand set.

What this file shows, and what the caps (train_cases.CAP, 64 for every family) rest on: every mutant of train_cases.MUTANTS moves some row of
every output it can reach by at least 3 x CAP = 192 yardsticks.  Measured on a build host (the smallest over the outputs of the best case per output):
    sparse     drop_last 1.1e6, dup_last 4.7e5, mask_shift 2.4e6 (dq, dK, dV; p > 0), kv_last_pair 7.5e5 (dK, dV)
    dense      drop_last 2.1e4, dup_last 7.1e3, mask_nk 2.0e5 (dq, dk, dv; p > 0, nk % 32 != 0), one lo product dropped 314 (ctx, a_lo b_hi) .. 576
    DN         drop_last 7.4e5, dup_last 4.4e5 in every case
    LayerNorm  mean(g) missing 4.1e4 (M = 1) .. 2.3e5
    colsum     a chunk's last row missing 3.9e4 .. 6.1e6 at every rows >= 1
    softmax    row sum over ld: 4.5e15 and more wherever ld > cols (inf at cols = 1, where dS is exactly 0)
The weakest is the dense format's own lo product, so the cap is the largest power of two below 314 / 3.  The fp32 yardsticks are fp32-class
(between 1e-8 and 1e-5); the dense model's lie between the fp32 evaluation's and 2^-10 (measured 7e-6 .. 1.4e-4 'plain', .. 7.8e-4 'sharp': dk of a
single sharp query)."""
import torch

import train_cases as tc

F64, F32 = torch.float64, torch.float32
SHOW = 3.0


def _show(family, name, score):
    print(f'{family} {name}: {score:.3g} yardsticks')
    assert score >= SHOW * tc.CAP[family], (family, name, score)


def test_bounds_respect_their_caps():
    assert set(tc.K) == set(tc.CAP) == {'sparse_fwd', 'sparse_bwd', 'dense_fwd', 'dense_bwd', 'self_attn_dn', 'ln_bwd', 'colsum', 'softmax_bwd'}
    for f, k in tc.K.items():
        assert k in (1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0) and k <= tc.CAP[f] == 64.0, (f, k)


# ------------------------------------------------------------------------------------------------ the cases are what they say
def test_sparse_csr_has_the_stated_lengths_and_pair_counts():
    rp, col = tc.sp_csr()
    assert rp.dtype == col.dtype == torch.int32 and rp.numel() == tc.SP_R + 1 == 35 and int(rp[0]) == 0 and int(rp[-1]) == col.numel()
    nk = (rp[1:] - rp[:-1]).tolist()
    lengths = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 203)
    assert tc.SP_S == 203 and tc.SP_S % 4 == 3 and tuple(nk[:17]) == lengths and tuple(nk[17:]) == lengths[::-1]
    assert tuple(r for r, n in enumerate(nk) if n == 0) == tc.SP_EMPTY_ROWS == (0, 33)
    assert int(col.min()) == 0 and int(col.max()) == tc.SP_S - 1                  # key 0 and key S - 1 are in use
    cnt = torch.bincount(col.long(), minlength=tc.SP_S)
    assert {k: int(cnt[k]) for k in (1, 2, 3, 4, 5)} == tc.SP_PAIR_COUNTS == {1: 1, 2: 3, 3: 4, 4: 5, 5: 9}
    assert int(cnt[tc.SP_SHARED_KEY]) == 32 and tc.SP_SHARED_KEY == 202
    for r in range(tc.SP_R):                                                      # ... one pair in every non-empty row
        assert int((col[rp[r]:rp[r + 1]] == tc.SP_SHARED_KEY).sum()) == (1 if nk[r] else 0)
    assert tuple((cnt == 0).nonzero().flatten().tolist()) == tc.SP_UNUSED_KEYS and len(tc.SP_UNUSED_KEYS) >= 8
    for r in range(tc.SP_R):                                                      # only the 203-key rows list a key twice
        assert (col[rp[r]:rp[r + 1]].unique().numel() == nk[r]) == (nk[r] != 203)
    for kind in ('plain', 'sharp'):
        c = tc.sp_case(kind)
        assert c.K.dtype == c.V.dtype == torch.bfloat16 and c.q.shape == (34, 256) and c.K.shape == (203, 256)
        assert 0.9 < float(c.q.std()) * 32.0 ** 0.5 / (3.0 if kind == 'sharp' else 1.0) < 1.1
    assert torch.equal(tc.sp_case('sharp').q, tc.sp_case('plain').q * 3.0) and tc.SP_DROPS == (0.0, 0.1, 0.5)


def test_sparse_drop_mask_is_the_numpy_restatement_of_the_library_wrapper():
    """sp_drop_mask restates ops.attn_drop_mask (itself numpy: importing it needs no library build)"""
    import numpy as np
    from mv2d_amd import ops
    nnz = tc.sp_case('plain').nnz
    for p in tc.SP_DROPS:
        assert np.array_equal(tc.sp_drop_mask(nnz, tc.SP_SEED, p), ops.attn_drop_mask(nnz, tc.SP_SEED, p))
    assert np.array_equal(tc.sp_drop_mask(nnz, 7, 0.5, shift=1)[:-1], ops.attn_drop_mask(nnz, 7, 0.5)[1:])
    m = tc.sp_drop_mask(nnz, tc.SP_SEED, 0.5)
    assert set(np.unique(m).tolist()) == {0.0, 2.0} and abs(float((m > 0).mean()) - 0.5) < 0.03


def test_dense_dn_and_reduction_cases_are_the_stated_ones():
    assert tc.DENSE_N == (1, 15, 16, 17, 33) and tc.DENSE_NK == (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257)
    p0 = {(n, nk) for n, nk, p in tc.DENSE_CASES if p == 0.0}
    pd = {(n, nk) for n, nk, p in tc.DENSE_CASES if p == 0.25}
    assert p0 == {(n, nk) for n in tc.DENSE_N for nk in tc.DENSE_NK} and len(tc.DENSE_CASES) == len(p0) + len(pd) == 65 + 21
    assert pd == {(17, nk) for nk in tc.DENSE_NK} | {(n, nk) for n in tc.DENSE_N for nk in (33, 257)}
    assert torch.equal(tc.dense_pool('sharp').q, tc.dense_pool('plain').q * 3.0) and torch.equal(tc.dense_pool('sharp').k, tc.dense_pool('plain').k)
    m = tc.dense_drop_mask(17, 33, 0.25, tc.DENSE_SEED)
    assert m.shape == (8, 17, 33) and abs(float((m > 0).mean()) - 0.75) < 0.03 and float(m.max()) == float(torch.tensor(1.0) / torch.tensor(0.75))
    assert tc.DN_CASES == ((33, 0, 1), (33, 33, 11), (48, 32, 16), (49, 34, 17), (50, 30, 15), (17, 16, 1), (65, 48, 3))
    for R, pad, single in tc.DN_CASES:
        vis = tc.dn_visible(R, pad, single)
        assert pad % max(single, 1) == 0 and pad <= R and bool(vis.any(1).all())
        assert bool(vis[pad:, pad:].all()) and not bool(vis[pad:, :pad].any())     # a matched query sees the matched queries only
        assert all(int(vis[r, :pad].sum()) == single for r in range(pad))          # a denoising query: its own group and the matched ones
    assert tc.LN_M == (0, 1, 3, 4, 5, 63, 64, 65, 129)
    for M in tc.LN_M[1:]:
        x = tc.ln_case(M).x
        assert float(x[0].var()) == 0.0 and float(x[M - 1].var()) == 0.0 and x.shape == (M, 256)
        for dt in (F32, F64):                                                      # variance 0 exactly in every evaluation
            assert float((x[[0, M - 1]].to(dt) - x[[0, M - 1]].to(dt).mean(1, keepdim=True)).abs().max()) == 0.0
    assert tc.CS_ROWS == (0, 1, 15, 16, 17, 63, 64, 65, 1024, 1025, 1537) and tc.CS_COLS == (1, 10, 16, 17, 256) and tc.CS_PAD == 3
    assert tc.SM_COLS == (1, 255, 256, 257, 1000) and tc.SM_PAD == 5
    c = tc.sm_case(257, True, True)
    assert c.ld == 262 and bool((c.P[:, 257:] == tc.SM_SENTINEL).all()) and bool((c.dP[:, 257:] == tc.SM_SENTINEL).all())
    assert 0.6 < float((c.Pd[:, :257] != 0).float().mean()) < 0.9 and abs(c.keep_scale - 4.0 / 3.0) < 1e-6


# ------------------------------------------------------------------------------------------------ yardsticks and mutants
def test_row_error_floor_and_exact_rows():
    want = torch.tensor([[0.0, 0.0], [4.0, -2.0], [1.0, 8.0]], dtype=F64)
    got = want + torch.tensor([[0.5, 0.0], [0.0, 1.0], [2.0, 0.0]], dtype=F64)
    assert tc.row_err(got, want).tolist() == [0.5 / 4.0, 1.0 / 4.0, 2.0 / 8.0]   # the median row maximum (4) floors the zero row
    z = torch.zeros(2, 3, dtype=F64)
    assert tc.row_err(z, z).tolist() == [0.0, 0.0] and tc.row_err(z + 1e-30, z).tolist() == [float('inf')] * 2
    assert tc.row_err(z + 1.0, z + 1e-20, mag=z + 4.0).tolist() == [0.25, 0.25]    # an output that vanishes to rounding: against its magnitude
    assert tc.row_err(z + 1.0, z + 2.0, mag=z + 4.0).tolist() == [0.5, 0.5]        # ... and only then
    assert tc.worst(got.masked_fill(torch.tensor([[True], [False], [False]]), float('nan')), want) == float('inf')
    assert tc.vec_err(torch.zeros(3), torch.zeros(3)) == 0.0 and tc.vec_err(torch.ones(3), torch.zeros(3)) == float('inf')


def test_sparse_yardsticks_and_mutants():
    for name in tc.SP_OUTPUTS:
        y = tc.sp_yard(name)
        print(f'sparse {name}: yardstick {y:.3e}')
        assert 1e-8 < y < 1e-5
    for p in tc.SP_DROPS:                                              # the listed rows: exactly 0 in the references themselves
        for kind in ('plain', 'sharp'):
            r = tc.sp_refs(kind, p)
            assert float(r.ctx[list(tc.SP_EMPTY_ROWS)].abs().max()) == 0.0 and float(r.dq[list(tc.SP_EMPTY_ROWS)].abs().max()) == 0.0
            assert float(r.dK[list(tc.SP_UNUSED_KEYS)].abs().max()) == 0.0 and float(r.dV[list(tc.SP_UNUSED_KEYS)].abs().max()) == 0.0
            one = [i for i, n in enumerate(tc.sp_case(kind).nk) if n == 1]
            assert float(r.dq[one].abs().max()) == 0.0                  # one key: the output does not depend on q
    reach = dict(drop_last=tc.SP_OUTPUTS, dup_last=tc.SP_OUTPUTS, mask_shift=('dq', 'dK', 'dV'), kv_last_pair=('dK', 'dV'))
    for mutant, outs in reach.items():
        best = dict.fromkeys(tc.SP_OUTPUTS, 0.0)
        for kind in ('plain', 'sharp'):
            for p in tc.SP_DROPS:
                ref, m = tc.sp_refs(kind, p), tc.sp_attend(kind, p, mutant=mutant)
                for name in tc.SP_OUTPUTS:
                    best[name] = max(best[name], tc.worst(getattr(m, name), getattr(ref, name)) / tc.sp_yard(name))
        for name in tc.SP_OUTPUTS:
            if name in outs:
                _show('sparse_fwd' if name == 'ctx' else 'sparse_bwd', f'{mutant} {name}', best[name])
            else:
                assert best[name] == 0.0, (mutant, name)


def test_dense_format_model_and_mutants():
    cases = [(n, nk, p, kd) for n, nk, p in tc.DENSE_CASES for kd in tc.dense_kinds(n, nk, p)]
    assert {kd for *_, kd in cases} == {'plain', 'sharp'}
    for kd in ('plain', 'sharp'):
        for name in tc.DENSE_OUTPUTS:
            y = tc.dense_yard(name, kd)
            f32 = max(tc.worst(getattr(tc.dense_attend(n, nk, p, kd, F32), name), getattr(tc.dense_refs(n, nk, p, kd), name),
                               mag=tc.dense_mag(tc.dense_refs(n, nk, p, kd), name)) for n, nk, p, k2 in cases if k2 == kd)
            print(f'dense {kd} {name}: format model {y:.3e}, fp32 evaluation {f32:.3e}')
            assert f32 < y < 2.0 ** -10                               # the format, not fp32 rounding, is what a correct kernel shows
    best = {}
    for n, nk, p, kd in cases:
        ref = tc.dense_refs(n, nk, p, kd)
        muts = {mu: tc.dense_attend(n, nk, p, kd, mutant=mu) for mu in (('drop_last', 'dup_last') if p == 0.0 else ('mask_nk',))}
        muts.update({'drop_' + d: tc.dense_attend(n, nk, p, kd, prod=tc.Bf16x3(d)) for d in ('a_lo', 'b_lo')})
        for mu, m in muts.items():
            for name in tc.DENSE_OUTPUTS:
                r = tc.worst(getattr(m, name), getattr(ref, name), mag=tc.dense_mag(ref, name)) / tc.dense_yard(name, kd)
                best[mu, name] = max(best.get((mu, name), 0.0), r)
    for (mu, name), r in best.items():
        if mu == 'mask_nk' and name in ('ctx', 'lse'):
            assert r == 0.0                                             # the forward's mask is the right one
        else:
            _show('dense_fwd' if name in ('ctx', 'lse') else 'dense_bwd', f'{mu} {name}', r)


def test_dense_one_key_gradients_vanish():
    """nk = 1: P = 1 and dS = dPd - D = 0, so dq and dk are zero to fp64 rounding and row_err measures them against their magnitude"""
    for n in tc.DENSE_N:
        ref = tc.dense_refs(n, 1, 0.0)
        assert float(ref.dq.abs().max()) <= 2.0 ** -40 * float(ref.dq_mag.abs().max()) and float(ref.dk.abs().max()) <= 2.0 ** -40 * float(ref.dk_mag.abs().max())
        assert float(tc.row_err(ref.dq + 1e-3 * ref.dq_mag, ref.dq, ref.dq_mag).max()) > 1e-4


def test_dn_yardstick_and_mutants():
    y = tc.dn_yard()
    print(f'self_attn_dn: yardstick {y:.3e}')
    assert 1e-8 < y < 1e-5
    for c in tc.DN_CASES:
        for mu in ('drop_last', 'dup_last'):
            _show('self_attn_dn', f'{mu} {c}', tc.worst(tc.dn_attend(*c, mutant=mu), tc.dn_refs(*c)) / y)
    assert torch.equal(tc.dn_attend(17, 16, 1)[:16], tc.dn_attend(17, 16, 1)[:16]) and tc.dn_refs(33, 0, 1).shape == (33, 256)


def test_reduction_yardsticks_and_mutants():
    for name in ('dx', 'dw', 'db'):
        y = tc.ln_yard(name)
        print(f'ln_bwd {name}: yardstick {y:.3e}')
        assert 1e-8 < y < 1e-5
    assert float(tc.ln_refs(0).dw.abs().max()) == 0.0 and float(tc.ln_refs(1).dw.abs().max()) == 0.0      # M = 1: a constant row, xhat = 0
    for M in tc.LN_M[1:]:
        _show('ln_bwd', f'no_mean_g M={M}', tc.worst(tc.ln_bwd(M, mutant='no_mean_g').dx, tc.ln_refs(M).dx) / tc.ln_yard('dx'))
    y = tc.cs_yard()
    print(f'colsum: yardstick {y:.3e}')
    assert 1e-8 < y < 1e-5
    for rows in tc.CS_ROWS:
        for cols in tc.CS_COLS:
            r = tc.vec_err(tc.colsum(rows, cols, mutant='chunk_last_row'), tc.colsum(rows, cols)) / y
            if rows:
                _show('colsum', f'chunk_last_row {rows}x{cols}', r)
            else:
                assert r == 0.0 and float(tc.colsum(0, cols).abs().max()) == 0.0 and torch.equal(tc.colsum(0, cols, add=True), tc.cs_pool()[1][:cols].double())
    y = tc.sm_yard()
    print(f'softmax_bwd: yardstick {y:.3e}')
    assert 1e-8 < y < 1e-5
    for cols in tc.SM_COLS:
        for dropped in (False, True):
            assert torch.equal(tc.softmax_bwd(cols, False, dropped), tc.softmax_bwd(cols, True, dropped))         # the pad columns do not enter
            assert tc.worst(tc.softmax_bwd(cols, False, dropped, mutant='rowsum_ld'), tc.softmax_bwd(cols, False, dropped)) == 0.0
            _show('softmax_bwd', f'rowsum_ld cols={cols} dropped={dropped}',
                  tc.worst(tc.softmax_bwd(cols, True, dropped, mutant='rowsum_ld'), tc.softmax_bwd(cols, True, dropped)) / y)
    assert float(tc.softmax_bwd(1, True, True).abs().max()) == 0.0
