"""The cases of tests/geometry_cases.py have teeth (CPU only).  Every defect the GPU tests of tests/test_gpu_geometry_edges.py are there to
catch is emulated in a variant of the oracle function (`_lists`, `_intr_variant`, `_rows_stopping` below; `_lists` without a defect IS the
oracle's epipolar_in_box, checked first) and must change the expected result of at least one case; the assertion messages carry the number of
RoIs that change.  The conditions that make the position-wise comparison of `match` meaningful are asserted as conditions.

On "a -1 gap before a valid entry".  Inside ONE (RoI, view) list the keep rule ((x > ratio * top) | (x > iou_thr)) & (x > 0) is monotone in x and
the list is sorted by x, descending: a kept entry can never follow a dropped one there (test_gap_conditions asserts this too).  The gaps a
consumer of `match` has to skip are those of a RoI's whole row [V * topk], which csr_count_kernel and csr_from_corr_block walk as one list: a
dropped entry at a rank INSIDE one view's list, followed by a kept entry of a later view.  That is the condition asserted per parameter set
with iou_thr > 0 -- except (iou_thr, ratio) = (1, 1), which keeps nothing at all (x > top and x > 1 are both impossible): there the condition
is that every list is dropped entirely.

On defect (c).  iou_thr compared with >= differs from > only where an IoU equals the threshold bit for bit (at iou_thr = 0 that is x = 0, which
`x > 0` drops anyway).  The `tight` box of the cases has IoU == 1.0f with the rectangle it was copied from, so the (1, 1) parameter set, which
keeps nothing under the rule, keeps that entry under >=."""
import functools

import numpy as np
import pytest
import torch

import geometry_cases as gc
from oracle import mv2d_oracle as O

DEFAULT_PS = gc.PARAM_SETS[0]


@functools.lru_cache(maxsize=None)
def _projected(name, sampling):
    """per sample (uv fp32 [R, V, N, 2], valid [R, V, N]) exactly as epipolar_in_box builds them"""
    ss, D, ds = sampling
    out = []
    for s in gc.make_case(name).samples:
        R, V = s.rois.size(0), gc.VIEWS
        pts = O.sample_points_in_rois(s.rois, ss)
        uv, valid = O.epipolar_in_each_view(pts.reshape(R * ss * ss, 3), s.metas[0]['pad_shape'], O.view_transforms(s.metas), D, ds, 70)
        out.append((uv.view(R, ss * ss, V, D, 2).permute(0, 2, 1, 3, 4).reshape(R, V, ss * ss * D, 2),
                    valid.view(R, ss * ss, V, D).permute(0, 2, 1, 3).reshape(R, V, ss * ss * D)))
    return out


def _lists(name, ps, defect=None):
    """epipolar_in_box (oracle/mv2d_oracle.py) with one defect of the kernel emulated; defect None: the oracle itself"""
    case, p = gc.make_case(name), gc.params(ps)
    sampling = (4, 8, 0.5) if defect == 'default_tables' else ps[:3]
    out = []
    for s, (uv, valid) in zip(case.samples, _projected(name, sampling)):
        starts = np.concatenate([[0], np.cumsum(s.npv)]).astype(int)
        rng = [(int(starts[v]), int(starts[v + 1])) for v in range(gc.VIEWS)]
        if defect == 'stale_view_range':
            passed_empty = False
            for v in range(gc.VIEWS):
                if passed_empty:
                    rng[v] = (int(starts[v - 1]), int(starts[v]))
                passed_empty |= s.npv[v] == 0
        for r in range(s.rois.size(0)):
            row = []
            for v in range(gc.VIEWS):
                lo, hi = rng[v]
                if hi == lo or not bool(valid[r, v].any()):
                    continue
                rv = s.rois[lo:hi]
                u, w_ = uv[r, v, :, 0], uv[r, v, :, 1]
                hit = ((rv[:, None, 1] <= u[None]) & (u[None] <= rv[:, None, 3]) & (rv[:, None, 2] <= w_[None]) & (w_[None] <= rv[:, None, 4]) &
                       valid[r, v][None])
                if not bool(hit.any()):
                    continue
                m = torch.ones_like(valid[r, v]) if defect == 'rect_all' else valid[r, v]
                pt = uv[r, v]
                pmax = torch.where(m[:, None], pt, torch.full_like(pt, -1e4)).max(0)[0]
                pmin = torch.where(m[:, None], pt, torch.full_like(pt, 1e4)).min(0)[0]
                iou = O.box_iou(torch.cat([pmin, pmax])[None], rv[:, 1:])[0]
                if defect == 'first_128':
                    iou = iou[:128]
                if defect == 'tie_high':
                    order = (iou.numel() - 1 - torch.argsort(iou.flip(0), descending=True, stable=True))[:p.topk]
                else:
                    order = torch.argsort(iou, descending=True, stable=True)[:p.topk]
                top = iou[order]
                if defect == 'no_ratio':
                    keep = (top > p.iou_thr) & (top > 0)
                elif defect == 'thr_ge':
                    keep = ((top > p.ratio * top.max()) | (top >= p.iou_thr)) & (top > 0)
                else:
                    keep = ((top > p.ratio * top.max()) | (top > p.iou_thr)) & (top > 0)
                row += [(i + lo + s.first, k) for i, k in zip(order.tolist(), keep.tolist())]
            out.append(row)
    return out


def _changed(name, ps, defect):
    """number of RoIs whose expected match rows change under the defect, and of those whose SET of kept ids changes"""
    case = gc.make_case(name)
    ref, _ = gc.expected_match(name, ps)
    got, _ = gc.match_from_lists(case, _lists(name, ps, defect), ps[5])
    rows = int((ref != got).view(case.R, -1).any(1).sum())
    sets = sum(set(a) != set(b) for a, b in zip(gc.rows_skipping_gaps(ref), gc.rows_skipping_gaps(got)))
    return rows, sets


@pytest.mark.parametrize('name', list(gc.LAYOUTS))
def test_variant_without_defect_is_the_oracle(name):
    for ps in gc.PARAM_SETS:
        assert _lists(name, ps) == gc.epipolar(name, ps), (name, ps)


def test_layouts():
    c = gc.make_case('mid_empty')
    assert c.npv[1] == 0 and max(c.npv) >= 257 and sorted(c.npv)[1] >= 129
    assert gc.make_case('first_empty').npv[0] == 0 and gc.make_case('last_empty').npv[-1] == 0
    assert [gc.make_case(n).R for n in ('r1', 'r127', 'r128', 'r129')] == [1, 127, 128, 129]
    b = gc.make_case('batch')
    assert b.B == 2 and b.view_start.numel() == 7 and tuple(b.trans.shape) == (6, 3, 16) and int(b.rois[:, 0].max()) == 4
    assert 0 in b.npv[:3] and 0 in b.npv[3:]
    for name in gc.LAYOUTS:
        c = gc.make_case(name)
        assert torch.equal(c.rois[:, 0].long(), torch.from_numpy(gc.view_of(c, np.arange(c.R)))) and int(c.view_start[-1]) == c.R
        for i, j in c.twins:
            assert torch.equal(c.rois[i], c.rois[j]) and i != j
    assert any(j - i > 128 for i, j in gc.make_case('mid_empty').twins)
    # the special boxes: integer corners at exactly min_size, the padded column, the image border
    c = gc.make_case('mid_empty')
    wh = c.rois[:, 3:5] - c.rois[:, 1:3]
    sp = {k: v[0] for k, v in c.special.items()}
    assert float(wh[sp['w4'], 0]) == 4.0 and float(wh[sp['h4'], 1]) == 4.0 and float(wh[sp['w16'], 0]) == 16.0 and float(wh[sp['h16'], 1]) == 16.0
    assert float(wh[sp['w3'], 0]) < 4 <= float(wh[sp['w3'], 1]) and float(wh[sp['h3'], 1]) < 4 <= float(wh[sp['h3'], 0])
    assert float(c.rois[sp['pad_col'], 1]) > gc.IMG_W - 1 and float(c.rois[sp['pad_col'], 3]) <= gc.PAD_W - 1
    assert gc.FOCAL * 7 / float(wh[sp['clamp'], 0]) > 5e3


def test_defect_a_first_128_rois_of_a_view():
    n = {ps: _changed('mid_empty', ps, 'first_128')[0] for ps in (gc.PARAM_SETS[0], gc.PARAM_SETS[2], gc.PARAM_SETS[3])}
    assert all(v > 0 for v in n.values()), f'RoIs changed when only the first 128 RoIs of a view are scored: {n}'
    print('defect a', n)


def test_defect_b_ties_towards_the_higher_index():
    res = {ps: _changed('mid_empty', ps, 'tie_high') for ps in (gc.PARAM_SETS[0], gc.PARAM_SETS[1], gc.PARAM_SETS[2], gc.PARAM_SETS[7])}
    assert all(rows > 0 for rows, _ in res.values()), f'(RoIs changed, RoIs with another kept set) under ties to the higher index: {res}'
    # the tie straddles the top-k cut (ranks topk - 1 and topk) where the SET of kept ids changes, not only its order
    assert res[gc.PARAM_SETS[1]][1] > 0 and res[gc.PARAM_SETS[7]][1] > 0, f'no positive-IoU tie across the cut at topk = 5 / 1: {res}'
    # ... and twins more than 128 indices apart are both kept in one list
    case = gc.make_case('mid_empty')
    far = [(i, j) for i, j in case.twins if j - i > 128]
    rows = gc.rows_skipping_gaps(gc.expected_match('mid_empty', gc.PARAM_SETS[0])[0])
    both = sum(any(i in row[1:] and j in row[1:] for i, j in far) for row in rows)
    assert both > 0, 'no list keeps both of two twins that lie more than 128 indices apart'
    print('defect b', res, 'rows with both far twins', both)


def test_defect_c_ratio_ignored():
    n = {ps: _changed(name, ps, 'no_ratio')[0] for name in ('mid_empty', 'r127') for ps in (gc.PARAM_SETS[1], gc.PARAM_SETS[3])}
    assert all(v > 0 for v in n.values()), f'RoIs changed when ratio is ignored: {n}'
    ge = {name: _changed(name, gc.PARAM_SETS[6], 'thr_ge')[0] for name in ('mid_empty', 'first_empty', 'r127')}
    assert all(v > 0 for v in ge.values()), f'RoIs changed when iou_thr = 1 is compared with >=: {ge}'
    print('defect c', n, '; iou_thr compared with >=:', ge)


def test_defect_d_rectangle_over_all_samples():
    n = {ps: _changed('mid_empty', ps, 'rect_all')[0] for ps in (gc.PARAM_SETS[0], gc.PARAM_SETS[4])}
    assert all(v > 0 for v in n.values()), f'RoIs changed when the rectangle takes the invalid samples too: {n}'
    print('defect d', n)


def test_defect_e_default_sampling_tables():
    n = {ps: _changed('mid_empty', ps, 'default_tables')[0] for ps in gc.PARAM_SETS if ps[:3] != (4, 8, 0.5)}
    assert len(n) == 5 and all(v > 0 for v in n.values()), f'RoIs changed when lin / depths / depth_start stay at their defaults: {n}'
    print('defect e', n)


def test_defect_f_view_range_after_an_empty_view():
    n = {name: _changed(name, DEFAULT_PS, 'stale_view_range')[0] for name in ('mid_empty', 'first_empty', 'batch')}
    assert all(v > 0 for v in n.values()), f'RoIs changed when the views behind an empty view read the previous range: {n}'
    assert _changed('last_empty', DEFAULT_PS, 'stale_view_range')[0] == 0          # (nothing lies behind the empty view there)
    print('defect f', n)


def _intr_variant(rois, K_roi, scale, min_size, defect):
    f = K_roi.view(-1, 16).clone().float() * scale
    wh = rois[:, 3:5] - rois[:, 1:3]
    f[(wh <= min_size).any(1) if defect == 'le' else (wh[:, 0] < min_size)] = 0
    return f.clamp(-5e3, 5e3)


def test_defect_g_min_size_and_the_small_and_clamp_conditions():
    case = gc.make_case('mid_empty')
    K = gc.box_params_ref(case)[0]
    n = {}
    for ms in (4, 16):
        ref = gc.intr_ref(case, K, 0.1, ms)
        for d in ('le', 'width_only'):
            n[(ms, d)] = int((_intr_variant(case.rois, K, 0.1, ms, d) != ref).any(1).sum())
    assert all(v > 0 for v in n.values()), f'intrinsics rows changed under (min_size, defect): {n}'
    print('defect g', n)
    # the small rows are zeroed under min_size = 4 and not under 0; the clamp is hit (and only without the zeroing)
    small = [r for k in gc.SMALL_4 for r in case.special[k]]
    assert bool((gc.intr_ref(case, K, 0.1, 4)[small] == 0).all()) and bool((gc.intr_ref(case, K, 0.1, 0)[small] != 0).any(1).all())
    kept = [r for k in ('w4', 'h4', 'w16') for r in case.special[k]]
    assert bool((gc.intr_ref(case, K, 0.1, 4)[kept] != 0).any(1).all())
    raw = O.process_intrins_feat(case.rois, K, 1.0, 0)
    hit = (raw.abs() > 5e3).any(1)
    assert bool(hit[case.special['clamp']].all()), 'intr_scale = 1 does not reach the 5e3 clamp on the quarter-pixel box'
    assert float(gc.intr_ref(case, K, 1.0, 0).abs().max()) == 5e3
    print('clamped rows', int(hit.sum()))


def _rows_stopping(match):
    """a consumer that stops at the first -1 of a RoI's row instead of skipping it"""
    m = match.view(match.shape[0], -1)
    rows = []
    for r in range(m.shape[0]):
        row = [r]
        for x in m[r].tolist():
            if x < 0:
                break
            row.append(x)
        rows.append(row)
    return rows


def _gap_rows(match, length):
    """(RoIs whose row has a dropped entry at a rank inside a view's list and a kept entry of a later view behind it,
        (RoI, view) lists in which a kept entry follows a dropped one)"""
    R, V, topk = match.shape
    kept = match >= 0
    inside = torch.arange(topk)[None, None] < length[..., None]
    dropped_v, kept_v = (~kept & inside).any(-1), kept.any(-1)                        # [R, V]
    before = (dropped_v.long().cumsum(1) - dropped_v.long()) > 0                      # a dropped entry in an earlier view's list
    within = (kept != (torch.arange(topk)[None, None] < kept.sum(-1, keepdim=True))).any(-1)
    return int((kept_v & before).any(1).sum()), int(within.sum())


def test_gap_conditions_and_defect_h_consumer_stops_at_a_gap():
    report = {}
    for ps in gc.PARAM_SETS:
        gaps = stops = kept = 0
        for name in gc.LAYOUTS:
            match, length = gc.expected_match(name, ps)
            g, within = _gap_rows(match, length)
            assert within == 0, 'the keep rule is monotone along a sorted list'
            gaps += g
            kept += int((match >= 0).sum())
            stops += sum(a != b for a, b in zip(gc.rows_skipping_gaps(match), _rows_stopping(match)))
        report[ps] = (gaps, stops)
        if ps[3:5] == (1.0, 1.0):
            assert kept == 0, f'{ps}: nothing can be kept'
        elif ps[3] > 0:
            assert gaps > 0, f'{ps}: no row with a dropped entry inside a list and a kept entry behind it'
            assert stops > 0, f'{ps}: a consumer that stops at the first -1 lists the same RoIs'
    assert sum(s for _, s in report.values()) > 0
    print('defect h: per parameter set (rows with a gap, rows a stopping consumer gets wrong)', report)


def test_lists_longer_and_shorter_than_topk():
    longer = shorter = 0
    for ps in gc.PARAM_SETS:
        for name in gc.LAYOUTS:
            case = gc.make_case(name)
            _, length = gc.expected_match(name, ps)
            n_v = torch.tensor([case.npv[(int(case.rois[r, 0]) // case.V) * case.V + v] for r in range(case.R) for v in range(case.V)]).view(case.R, case.V)
            hitl = length > 0
            assert bool((length[hitl] == n_v[hitl].clamp(max=ps[5])).all())
            longer += int((hitl & (n_v > ps[5])).sum())
            shorter += int((hitl & (n_v < ps[5])).sum())
    assert longer > 0 and shorter > 0, (longer, shorter)


def test_an_empty_csr_row_exists():
    empty = {}
    for topk, expand, ps in ((1, 0, gc.PARAM_SETS[7]), (20, 2, gc.PARAM_SETS[0])):
        ffr, pad = gc.t_path_ref('mid_empty', ps, expand)
        allowed = (ffr & ~pad[None]).view(ffr.shape[0], -1)
        empty[(topk, expand)] = int((allowed.sum(1) == 0).sum())
    assert all(v > 0 for v in empty.values()), f'empty CSR rows per (topk, expand): {empty}'
    case = gc.make_case('mid_empty')
    assert not bool(allowed[case.special['out_below']].any())


@pytest.mark.parametrize('name', list(gc.LAYOUTS))
def test_projection_is_the_same_in_the_kernels_operation_order(name):
    """The exact comparison does not hang on the accumulation order of torch.matmul: the kernel's order -- acc = 0, acc = acc + T[i][k] * x_k for
    k = 0 .. 3, no contraction -- gives the oracle's uv bit for bit on every case (a seed that ever breaks this is changed, not the comparison)."""
    total = 0
    for sampling in sorted({ps[:3] for ps in gc.PARAM_SETS}):
        ss, D, ds = sampling
        for s, (uv, _) in zip(gc.make_case(name).samples, _projected(name, sampling)):
            R = s.rois.size(0)
            if R == 0:
                continue
            T = O.view_transforms(s.metas)[s.rois[:, 0].long()]                                    # [R, V, 4, 4]
            lin = torch.linspace(0, 1, ss)
            wh = s.rois[:, 3:5] - s.rois[:, 1:3]
            x = (s.rois[:, 1, None] + wh[:, 0, None] * lin[None])[:, None, :].expand(R, ss, ss).reshape(R, ss * ss)
            y = (s.rois[:, 2, None] + wh[:, 1, None] * lin[None])[:, :, None].expand(R, ss, ss).reshape(R, ss * ss)
            d = O.lid_depths(D, ds, 70).double()
            hx = (x.double()[:, :, None] * d).reshape(R, 1, -1)
            hy = (y.double()[:, :, None] * d).reshape(R, 1, -1)
            dd = d[None, None].expand(R, ss * ss, D).reshape(R, 1, -1)
            cam = []
            for i in range(3):
                acc = torch.zeros_like(hx).expand(R, gc.VIEWS, hx.shape[-1])
                acc = acc + T[:, :, i, 0, None] * hx
                acc = acc + T[:, :, i, 1, None] * hy
                acc = acc + T[:, :, i, 2, None] * dd
                acc = acc + T[:, :, i, 3, None] * 1.0
                cam.append(acc)
            z = cam[2].clamp_min(1e-2)
            mine = torch.stack([cam[0] / z, cam[1] / z], -1).float()
            assert torch.equal(mine.view(torch.int32), uv.view(torch.int32)), (name, sampling)
            total += mine.numel()
    print(name, 'uv values compared', total)
