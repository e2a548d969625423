"""The cases of tests/xattn_cases.py have teeth (CPU only): on the shared-hi rows every defect of the lo terms that the GPU tests are there
to catch, emulated in torch fp64, moves the results of the rows it touches by at least half of what the lo halves contribute, while a plain
fp32 evaluation of the same operands stays 64 times below the smallest of them.  That factor is the room tests/test_gpu_xattn_lo.py has for
its bound k (kernel error <= k x the fp32 evaluation's error, k <= 64)."""
import functools

import pytest
import torch

import xattn_cases as xc

SEED = {0: 2100, 6: 2106}
DEFECT_FLOOR, YARDSTICK_ROOM = 0.5, 64.0


@functools.lru_cache(maxsize=None)
def _setup(e):
    case = xc.shared_hi_case(e, SEED[e])
    khi, klo = xc.split_key16(case.xk32)
    vhi, vlo = xc.split_key16(case.xv32)
    Qt = xc.qt_emulated(case)
    ref = xc.attend(case, Qt, khi, klo, vhi, vlo)
    return case, (khi, klo, vhi, vlo), Qt, ref


def _errors(case, ref, res):
    """per row: (error of the centred logits, error of z - h_v, error of ctx - (Wv h_v + bv))"""
    zb, cb = xc.bases(case, lo_free=False)
    return xc.logit_row_errors(case, res.logits, ref.logits, centre=True), xc.row_errors(res.z, ref.z, zb), xc.row_errors(res.ctx, ref.ctx, cb)


def _defects(case, ops, Qt):
    """name -> (result of the defective evaluation, rows [R] bool that the defect touches)"""
    khi, klo, vhi, vlo = ops
    many = case.nk >= 2
    pos, nk_pair = case.pair_pos, case.nk[case.pair_row]
    ragged = pos < nk_pair // xc.TILE * xc.TILE                      # False for the last nk mod 16 pairs of a row
    ntile = (nk_pair + xc.TILE - 1) // xc.TILE
    tile = pos // xc.TILE
    last_wave = (tile % 4) != ((ntile - 1) % 4)                      # 4 waves, tiles dealt round robin: the wave that takes the last tile
    first_wave = (tile % 4) != 0
    k8, v8 = xc.lo8_encode(klo), xc.lo8_encode(vlo)
    at = functools.partial(xc.attend, case, Qt)
    return {
        'key lo dropped': (at(khi, None, vhi, vlo), many),
        'value lo dropped': (at(khi, klo, vhi, None), many),
        'key lo rolled by 8 channels': (at(khi, klo.roll(8, 1), vhi, vlo), many),
        'value lo rolled by 8 channels': (at(khi, klo, vhi, vlo.roll(8, 1)), many),
        'lo of the ragged last tile dropped': (at(khi, klo, vhi, vlo, keep_k=ragged, keep_v=ragged), many & (case.nk % xc.TILE != 0)),
        'lo of the wave with the last tile dropped (4 waves)': (at(khi, klo, vhi, vlo, keep_k=last_wave, keep_v=last_wave), many),
        'lo of the first wave dropped (4 waves)': (at(khi, klo, vhi, vlo, keep_k=first_wave, keep_v=first_wave), many),
        'lo8 scale taken as 2^11': (at(khi, xc.lo8_decode(k8, 2048.0), vhi, xc.lo8_decode(v8, 2048.0)), many),
    }


@pytest.mark.parametrize('e', [0, 6])
def test_shared_hi_construction(e):
    """hi of every key of a row is one bit pattern (== the shared h), the lo halves stay inside the NORMAL range of the e4m3 "lo8" bytes (no
    saturation, no subnormal byte: the producers' lo8 flag must stay 0), the logit spread has a standard deviation of 1 .. 2 per (row, head)."""
    case, (khi, klo, vhi, vlo), Qt, ref = _setup(e)
    for b in range(0, case.R, 8):                                                                      # every block of 8 queries mixes short and long rows
        assert int(case.nk[b:b + 8].min()) <= 17 and int(case.nk[b:b + 8].max()) >= 63
    assert set(xc.ROW_LENGTHS) <= set(case.nk.tolist()) and case.R == len(xc.ROW_LENGTHS) + 3 and case.S <= 2500
    rp, col = case.row_ptr.tolist(), case.col_idx.long()
    strided = col[rp[xc.STRIDED_ROW]:rp[xc.STRIDED_ROW + 1]]
    assert len(strided) == xc.STRIDED_KEYS and bool((strided[1:] - strided[:-1] == xc.STRIDE).all())
    shared = [r for r in range(case.R) if any(r != s and rp[r + 1] > rp[r] and torch.equal(col[rp[r]:rp[r + 1]], col[rp[s]:rp[s + 1]]) for s in range(case.R))]
    assert tuple(shared) == xc.SHARED_ROWS
    for r in range(case.R):
        cols = col[rp[r]:rp[r + 1]]
        if len(cols):
            assert torch.equal(khi[cols].view(torch.int16), case.hk[r].to(torch.float16).view(torch.int16).expand(len(cols), -1)), r
            assert torch.equal(vhi[cols].view(torch.int16), case.hv[r].to(torch.float16).view(torch.int16).expand(len(cols), -1)), r
    assert bool((case.hk.to(torch.float16).float() == case.hk).all()) and bool((case.hv.to(torch.float16).float() == case.hv).all())
    for lo in (klo, vlo):
        s = lo.float().abs() * xc.LO8_SCALE
        assert float(s.min()) >= 2.0 ** -6 and float(s.max()) <= 448.0
        assert int(((xc.lo8_encode(lo) & 0x7f) < 8).sum()) == 0                                          # no subnormal byte
        assert float((xc.lo8_decode(xc.lo8_encode(lo)).float() - lo.float()).abs().max()) <= float(lo.float().abs().max()) * 2.0 ** -4
    for r in range(case.R):
        if case.nk[r] >= 2:
            std = ref.logits[:, rp[r]:rp[r + 1]].std(1, unbiased=False)
            assert 1.0 <= float(std.min()) and float(std.max()) <= 2.0, (r, std)
            # without the lo halves every key of the row has the same logit and z == h_v
    flat = xc.attend(case, Qt, khi, None, vhi, None)
    for r in range(case.R):
        if case.nk[r] >= 1:
            assert float((flat.logits[:, rp[r]:rp[r + 1]] - flat.logits[:, rp[r]:rp[r] + 1]).abs().max()) == 0.0
            assert float((flat.z[r] - case.hv[r].double()).abs().max()) <= 2.0 ** -40 * float(case.hv[r].abs().max())      # fp64 row sums


@pytest.mark.parametrize('e', [0, 6])
def test_emulated_defects_show_and_fp32_does_not(e):
    """Every emulated defect gives an error >= 0.5 on every row it touches (rows of two or more keys; for the ragged tile those whose length is
    no multiple of 16), and that error is at least 64 times the largest error of a plain fp32 evaluation of the same operands in the same quantity
    (the yardstick of the GPU test, which allows a kernel k <= 64 times it).  The defects of a whole side are held on z - h_v alone, and show in ctx
    as well; the three that drop the lo halves of SOME keys of a row are held on the logits or on z, whichever shows them -- one key among 257
    carries at most its probability of z, but its own logit in full, and the GPU test holds both quantities per row.  ctx = Wv z + bv has less
    room: the fp32 rounding of Wv h_v is charged to Wv (z - h_v), so there the whole-side defects (>= 0.5) are held to 16 yardsticks, twice the
    GPU test's K = 8, and the 64 come through z, which the fused kernel's ctx equals bit for bit after the context map."""
    case, ops, Qt, ref = _setup(e)
    khi, klo, vhi, vlo = ops
    lg, z, ctx = _errors(case, ref, xc.attend(case, Qt, khi, klo, vhi, vlo, dtype=torch.float32))
    has = case.nk >= 1
    yard_lg, yard_z, yard_ctx = float(lg[case.nk >= 2].max()), float(z[has].max()), float(ctx[has].max())
    print(f'e={e} fp32 evaluation, largest row error: logits {yard_lg:.2e}, z {yard_z:.2e}, ctx {yard_ctx:.2e}')
    assert yard_lg * YARDSTICK_ROOM <= DEFECT_FLOOR                  # the floor itself is out of a correct kernel's reach, with room ...
    assert yard_ctx * 16.0 <= DEFECT_FLOOR
    for name, (res, rows) in _defects(case, ops, Qt).items():
        lg, z, ctx = _errors(case, ref, res)
        assert int(rows.sum()) >= 14
        shows_z = z >= max(DEFECT_FLOOR, YARDSTICK_ROOM * yard_z)    # ... and so is 64 x the yardstick where that is the larger one
        shows_lg = lg.nan_to_num(0.0) >= max(DEFECT_FLOOR, YARDSTICK_ROOM * yard_lg)
        partial = name.startswith('lo of the')
        print(f'e={e} {name}: smallest row error in z {float(z[rows].min()):.3f}, logits {float(lg[rows].min()):.3f}, ctx {float(ctx[rows].min()):.3f}')
        assert bool((shows_z | shows_lg if partial else shows_z)[rows].all()), (name, lg, z)
        if not partial:
            assert float(ctx[rows].min()) >= DEFECT_FLOOR, (name, ctx)


def test_random_case_shapes():
    """The random case: the same CSR, unit-variance rows whose lo halves are ordinary fp16 remainders, one sharp query on a row of 129 keys."""
    case, sh = xc.random_case(2200), xc.shared_hi_case(0, SEED[0])
    assert case.nk.tolist() == sh.nk.tolist() and case.S == sh.S
    r = case.nk.tolist().index(129)
    others = torch.cat([case.q[:r], case.q[r + 1:]])
    assert float(case.q[r].std()) > 6.0 * float(others.std())                          # the one sharp query
    khi, klo = xc.split_key16(case.xk32)
    assert float((khi.double() + klo.double() - case.xk32.double()).abs().max()) <= 2.0 ** -21 * float(case.xk32.abs().max())
