"""The cases of tests/tail_cases.py have teeth (CPU only).  The references the GPU tests of tests/test_gpu_tail_edges.py compare with are pinned to
oracle/mv2d_oracle.py first: decode_ranked IS O.decode wherever the selected scores are distinct, `_pack` and `_nms` below without a defect ARE
O.post_nms_pack and O.nms_bev.  Then every defect the GPU tests are there to catch is emulated in a variant of the reference and must change
the expected result of at least one named case; the assertion messages carry the number of entries that change.  The conditions that make the
exact comparison of the NMS keep masks meaningful (no same-class IoU within tail_cases.IOU_MARGIN of the threshold, 20 % .. 80 % kept) are
asserted as conditions.

The wire format: mv2d_amd.dist.pack_detections writes the count field as it is handed in, NOT clamped to max_num (rows are clamped, the
count is not); that is what the `count_clamped` variant departs from."""
import functools

import numpy as np
import pytest
import torch

import tail_cases as tc
from mv2d_amd import dist as mdist
from oracle import mv2d_oracle as O


def _same(a, b):
    """bit-equal tuples of tensors, NaN equal to NaN"""
    return all(x.shape == y.shape and x.dtype == y.dtype and bool(((x == y) | ((x != x) & (y != y))).all()) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ decode
def _decode(c, defect=None):
    """decode_ranked with one defect of the kernel emulated: (boxes, scores, labels, bbox_index, count)"""
    img = tc.key_image(c.cls).astype(np.int64)
    n, K = img.size, min(c.max_num, img.size)
    ids = np.arange(n)
    if defect == 'tie_high':
        idx = np.lexsort((-ids, -img))[:K]
    elif defect == 'overflow_reversed':
        # the kernel before the fix: every key whose logit image is >= the K-th takes a slot in arrival order (here: highest index first) and
        # only the first 1024 are stored; the stored ones are ranked
        kth = np.sort(img)[::-1][K - 1]
        stored = ids[img >= kth][::-1][:1024]
        idx = stored[np.lexsort((stored, -img[stored]))][:K]
    elif defect == 'k_max_num':
        idx = np.argsort(-img, kind='stable')[:K]
        idx = np.concatenate([idx, np.zeros(c.max_num - K, dtype=idx.dtype)])        # ranks n .. max_num read some in-range candidate
    else:
        idx = np.argsort(-img, kind='stable')[:K]
    idx = torch.from_numpy(idx.copy())
    out = tc.emit(c.cls, c.reg, idx, c.N, torch.gt, torch.lt) if defect == 'strict_range' else tc.emit(c.cls, c.reg, idx, c.N)
    if defect == 'no_z_shift':
        b = out[0].clone()
        b[:, 2] = b[:, 2] + b[:, 5] * 0.5
        out = (b,) + tuple(out[1:])
    count = idx.numel() if defect == 'count_before_filter' else out[0].shape[0]
    return out + (count,)


def _decode_changed(c, defect):
    """number of output entries (ranked flat indices, box rows, the count) a defect changes in a case"""
    a, b = _decode(c), _decode(c, defect)
    fa, fb = (a[3] * c.N + a[2]).tolist(), (b[3] * c.N + b[2]).tolist()
    m = max(len(fa), len(fb))
    fa, fb = fa + [-1] * (m - len(fa)), fb + [-1] * (m - len(fb))
    changed = sum(x != y for x, y in zip(fa, fb)) + int(a[4] != b[4])
    if a[0].shape == b[0].shape:
        changed += int((a[0] != b[0]).any(1).sum())
    return changed


def test_decode_ranked_is_the_oracle_where_scores_are_distinct():
    pinned = 0
    for name in tc.DECODE_CASES:
        c = tc.decode_case(name)
        exp = tc.decode_expected(name)
        assert _same(exp, _decode(c)[:4])
        sel = c.cls.sigmoid().view(-1)[tc.rank_flat(c.cls, c.max_num + 1)]                # the selected scores and the first one left out
        distinct = not bool(torch.isnan(sel).any()) and torch.unique(sel).numel() == sel.numel()
        if name in tc.DECODE_SIZES or name in tc.DECODE_RANGE:
            assert distinct, f'{name}: the selected scores of a distinct-logit case collide'
        if distinct:
            ref = O.decode(c.cls, c.reg, c.max_num, c.N)
            assert _same(exp, ref), name
            pinned += 1
    assert pinned >= len(tc.DECODE_SIZES) + len(tc.DECODE_RANGE)
    g = tc.group_case()
    for (a, b), exp in zip(zip(g.grp_start[:-1].tolist(), g.grp_start[1:].tolist()), g.expected[:3]):
        if b > a:
            assert _same(exp, O.decode(g.cls[a:b], g.reg[a:b], g.max_num, g.N))


def test_decode_cases_are_what_they_claim():
    flat = lambda name: (tc.decode_expected(name)[3] * tc.decode_case(name).N + tc.decode_expected(name)[2]).tolist()
    assert flat('mass_tie_lds') == list(range(300))
    c = tc.decode_case('boundary_tie')
    f = flat('boundary_tie')
    assert len(f) == 1024 and min(c.pair) in f and max(c.pair) not in f and f[-1] == min(c.pair)
    img = tc.key_image(c.cls)
    assert int((img >= np.sort(img)[::-1][1023]).sum()) == 1025                       # one more survivor than slots
    c = tc.decode_case('partial_tie')
    f = flat('partial_tie')
    v = c.cls.reshape(-1)
    assert bool((v[f[:100]] > 0.5).all()) and bool((v[f[:100]][:-1] > v[f[:100]][1:]).all()) and f[100:] == c.plateau[:200].tolist()
    f = flat('mass_tie_stream')
    last = 300 * 64 - 1
    assert f[:5] == [last, 4097, 15000, 9000, 0] and f[5:] == [i for i in range(1, 400) if i not in tc.MASS_STREAM_TOP][:295]
    c = tc.decode_case('nan_group')
    assert flat('nan_group') == c.nan_idx[:300].tolist() and bool(torch.isnan(tc.decode_expected('nan_group')[1]).all())
    top = torch.topk(c.cls.reshape(-1), 300)[0]
    assert bool(torch.isnan(top).all())                                               # torch.topk ranks NaN largest too
    c = tc.decode_case('adjacent_floats')
    sel = c.cls.reshape(-1)[tc.rank_flat(c.cls, 300)]
    assert torch.unique(sel).numel() > torch.unique(sel.sigmoid()).numel()            # sigmoid collapses neighbours
    c = tc.decode_case('sign_and_specials')
    img = tc.key_image(c.cls).astype(np.int64)
    order = np.argsort(-img, kind='stable')
    vals = c.cls.reshape(-1).numpy()[order].astype(np.float64)
    assert (vals[:-1] >= vals[1:]).all() and vals[0] == np.inf and vals[-1] == -np.inf
    sb = np.signbit(c.cls.reshape(-1).numpy()[order])[vals == 0.0]
    assert sb.size == 4 and list(sb) == sorted(sb)                                    # +0 ranks above -0
    ref = O.decode(c.cls, c.reg, c.max_num, c.N)
    assert sorted(flat('sign_and_specials')) == sorted((ref[3] * c.N + ref[2]).tolist())
    # range filter: centres ON a bound kept, one ulp outside dropped
    c = tc.decode_case('range_edges')
    kept_rows = set(tc.decode_expected('range_edges')[3].tolist())
    assert set(c.on) <= kept_rows and not (set(c.off) & kept_rows) and len(kept_rows) == tc.RANGE_ROWS - 6
    assert tc.decode_expected('range_all_dropped')[0].shape[0] == 0 and tc.decode_expected('range_none_dropped')[0].shape[0] == 300
    g = tc.group_case()
    assert [e[0].shape[0] > 0 for e in g.expected] == [True, False, True, True] and g.expected[0][0].shape[0] <= 10
    a = int(g.grp_start[3])
    assert (g.expected[3][3] * g.N + g.expected[3][2]).tolist()[:5] == [0, 1, 2, 3, 4] and bool((g.cls[a:] == g.cls[a, 0]).all())


DECODE_DEFECTS = {
    'overflow_reversed': ('boundary_tie', 'partial_tie', 'mass_tie_lds', 'mass_tie_stream', 'nan_group'),
    'tie_high': ('mass_tie_lds', 'boundary_tie', 'partial_tie', 'mass_tie_stream', 'nan_group', 'adjacent_floats', 'sign_and_specials'),
    'k_max_num': ('n70',),
    'strict_range': ('range_edges',),
    'count_before_filter': ('range_edges', 'range_all_dropped', 'n300'),
    'no_z_shift': ('n1024', 'range_none_dropped'),
}


@pytest.mark.parametrize('defect', list(DECODE_DEFECTS))
def test_decode_defects_change_the_expected_result(defect):
    for name in DECODE_DEFECTS[defect]:
        changed = _decode_changed(tc.decode_case(name), defect)
        assert changed > 0, f'{defect} changes {changed} entries of {name}'


def test_overflow_defect_leaves_the_cases_without_overflow_alone():
    for name in tc.DECODE_SIZES:
        assert _decode_changed(tc.decode_case(name), 'overflow_reversed') == 0, name


# ------------------------------------------------------------------------------------------------ pack
def _pack(c, defect=None):
    """post_nms_pack as result_pack_kernel computes it (rank by (label, -score, index) or, beyond max_num survivors, a stable score sort of
    that list), with one defect emulated"""
    n = c.stride if defect == 'read_beyond_count' else c.count
    s, l_ = c.scores[:n].numpy(), c.labels[:n].numpy()
    keep = np.nonzero(s >= c.score_thr if defect == 'ge_thr' else s > c.score_thr)[0]
    order = keep[np.lexsort((keep, -s[keep], l_[keep]))]                              # class-major, score descending, index ascending
    over = len(order) > c.max_num
    if defect == 'class_major_always':
        order = order[:c.max_num]
    elif over or defect == 'global_always':
        order = order[np.argsort(-s[order], kind='stable')][:c.max_num]
    order = torch.from_numpy(order.copy())
    return c.boxes[order], c.scores[order], c.labels[order]


def _pack_changed(c, defect):
    a, b = _pack(c), _pack(c, defect)
    if a[1].shape != b[1].shape:
        return abs(a[1].shape[0] - b[1].shape[0]) + int((a[1][:min(len(a[1]), len(b[1]))] != b[1][:min(len(a[1]), len(b[1]))]).sum())
    return int(((a[1] != b[1]) | (a[2] != b[2]) | ~((a[0] == b[0]) | (torch.isnan(a[0]) & torch.isnan(b[0]))).all(1)).sum())


def _all_pack_cases():
    return [tc.pack_case(n) for n in tc.PACK_CASES] + list(tc.pack_batch_case().samples)


def test_pack_reference_is_the_oracle():
    for c in _all_pack_cases():
        exp = tc.pack_expected(c)
        assert _same(exp, _pack(c)), c.name
        assert bool(torch.isfinite(exp[0]).all()) and bool((exp[2] < c.num_classes).all()), f'{c.name}: garbage in the expectation'
    assert [tc.pack_expected(tc.pack_case(n))[1].shape[0] for n in ('count0', 'count1', 'count1024', 'survivors_eq_max', 'survivors_max_plus1',
                                                                   'ones_over', 'nan_inf')] == [0, 1, 1024, 300, 300, 300, 100]
    lab = tc.pack_expected(tc.pack_case('survivors_eq_max'))[2]
    assert bool((lab[1:] >= lab[:-1]).all())                                          # class-major at exactly max_num survivors
    lab = tc.pack_expected(tc.pack_case('survivors_max_plus1'))[2]
    assert not bool((lab[1:] >= lab[:-1]).all())                                      # global score order one survivor later
    c = tc.pack_case('thr_equal')
    got = set(tc.pack_expected(c)[1].tolist())
    assert float(tc.THR) not in got and float(np.nextafter(tc.THR, np.float32(1), dtype=np.float32)) in got
    assert int(tc.pack_expected(tc.pack_case('count1024'))[2].max()) == 63
    lab = tc.pack_expected(tc.pack_case('ones_over'))[2]
    assert bool((lab[1:] >= lab[:-1]).all()) and int(lab.max()) == 9                  # equal scores beyond max_num: the class-major list's order


PACK_DEFECTS = {
    'class_major_always': ('survivors_max_plus1',),
    'global_always': ('survivors_eq_max', 'count1024'),
    'ge_thr': ('thr_equal',),
    'read_beyond_count': ('count0', 'count1', 'nan_inf', 'batch0', 'batch1', 'batch2'),
}


@pytest.mark.parametrize('defect', list(PACK_DEFECTS))
def test_pack_defects_change_the_expected_result(defect):
    by_name = {c.name: c for c in _all_pack_cases()}
    for name in PACK_DEFECTS[defect]:
        changed = _pack_changed(by_name[name], defect)
        assert changed > 0, f'{defect} changes {changed} entries of {name}'


# ------------------------------------------------------------------------------------------------ wire
def _wire(c, defect=None):
    out = []
    for b in range(c.count.numel()):
        n = min(int(c.count[b]), c.max_num)
        rows = torch.cat([c.boxes[b, :c.max_num], c.scores[b, :c.max_num, None], c.labels[b, :c.max_num, None].float()], 1)
        if defect != 'not_zeroed':
            rows[n:] = 0.0
        cnt = float(n if defect == 'count_clamped' else int(c.count[b]))
        out.append(torch.cat([rows.reshape(-1), torch.tensor([cnt])]))
    return torch.stack(out)


def test_wire_reference_round_trip_and_defects():
    c = tc.wire_case()
    assert c.expected.shape == (len(tc.WIRE_COUNTS), c.max_num * 11 + 1) and bool(torch.isfinite(c.expected).all())
    assert torch.equal(c.expected, _wire(c))
    for b, cnt in enumerate(tc.WIRE_COUNTS):
        assert torch.equal(c.expected[b], mdist.pack_detections(c.boxes[b], c.scores[b], c.labels[b], c.count[b:b + 1], c.max_num))
        assert float(c.expected[b, -1]) == cnt                                        # the count field is not clamped
        n = min(cnt, c.max_num)
        bx, sc, lb = mdist.unpack_detections(c.expected[b], c.max_num)
        assert torch.equal(bx, c.boxes[b, :n]) and torch.equal(sc, c.scores[b, :n]) and torch.equal(lb, c.labels[b, :n])
        assert bool((c.expected[b, n * 11:-1] == 0).all())
        assert n == 0 or int(lb.max()) == 63
    for defect in ('not_zeroed', 'count_clamped'):
        v = _wire(c, defect)
        changed = int((~((v == c.expected) | (torch.isnan(v) & torch.isnan(c.expected)))).sum())
        assert changed > 0, f'{defect} changes {changed} payload words'


# ------------------------------------------------------------------------------------------------ NMS
@functools.lru_cache(maxsize=None)
def _ious(name):
    """fp64 IoU of EVERY pair of a small case (cross-class pairs too)"""
    c = tc.nms_case(name)
    b = c.boxes.numpy().astype(np.float64)
    m = np.zeros((c.n, c.n))
    for i in range(c.n):
        for j in range(i + 1, c.n):
            m[i, j] = m[j, i] = O.rotated_iou_bev(b[j], b[i])
    return m


def _nms(name, defect=None):
    c = tc.nms_case(name)
    iou, s, l_ = _ious(name), c.scores.numpy().astype(np.float64), c.labels.numpy()
    ids = np.arange(c.n)
    order = np.lexsort((-ids, -s)) if defect == 'tie_high' else np.argsort(-s, kind='stable')
    keep = np.ones(c.n, bool)
    for a_, i in enumerate(order):
        if not keep[i] and defect != 'dead_suppresses':
            continue
        for j in order[a_ + 1:]:
            if l_[j] != l_[i] and defect != 'cross_class':
                continue
            if keep[j] and (iou[j, i] >= c.thr if defect == 'ge_thr' else iou[j, i] > c.thr):
                keep[j] = False
    return torch.from_numpy(keep)


SMALL_NMS = tuple(n for n in tc.NMS_CASES if n not in tc.NMS_RANDOM)


def test_nms_reference_is_the_oracle_and_cases_are_what_they_claim():
    for name in SMALL_NMS:
        assert torch.equal(_nms(name), tc.nms_expected(name)), name
    e = lambda name: tc.nms_expected(name).tolist()
    assert e('n0') == [] and e('n1') == [True] and e('n2') == [False, True]
    assert e('identical') == [False, True, False, False, True, False, False]
    assert e('nested_in') == [True, False] and e('nested_out') == [True, True]
    assert e('touching') == [True] * 5 and e('zero_area') == [True] * 5 + [False]
    assert e('yaws') == [True, False, False, True, False, True, True]
    assert e('chain') == [True, False, True]                                          # scores C > B > A: C kills B, A (IoU 1/3 with C) stays
    assert e('cross_class') == [True, True, True, False]
    assert e('score_ties')[0] and not e('score_ties')[1]
    assert e('thr_one') == [True] * 3
    for cf, a, b, iou in tc.CLOSED_FORMS:
        assert abs(O.rotated_iou_bev(np.asarray(a), np.asarray(b)) - iou) < 1e-12
        assert e(cf + '_below') == [True, False] and e(cf + '_above') == [True, True]


NMS_DEFECTS = {
    'cross_class': ('cross_class',),
    'ge_thr': ('thr_one', 'touching'),
    'dead_suppresses': ('chain',),
    'tie_high': ('score_ties', 'identical'),
}


@pytest.mark.parametrize('defect', list(NMS_DEFECTS))
def test_nms_defects_change_the_expected_result(defect):
    for name in NMS_DEFECTS[defect]:
        changed = int((_nms(name, defect) != tc.nms_expected(name)).sum())
        assert changed > 0, f'{defect} changes {changed} keep flags of {name}'


def _margin_and_share(boxes, scores, labels, thr, keep, what):
    ious = np.asarray(list(tc.same_class_ious(boxes.numpy(), labels.numpy()).values()))
    gap = float(np.abs(ious - thr).min())
    share = float(keep.float().mean())
    assert gap > tc.IOU_MARGIN, f'{what}: a same-class IoU {gap:.2e} from thr'
    assert 0.2 <= share <= 0.8, f'{what}: {share:.0%} kept'
    assert float(boxes[:, :2].abs().max()) <= 25.0 and float((boxes[:, 3] * boxes[:, 4]).min()) >= 2.25


def test_random_nms_cases_keep_their_margin_and_kept_share():
    for name in tc.NMS_RANDOM:
        c = tc.nms_case(name)
        _margin_and_share(c.boxes, c.scores, c.labels, c.thr, tc.nms_expected(name), name)
    assert tc.nms_case('big1024').n == 1024 and int(tc.nms_case('big1024').labels.max()) == 15
    bc = tc.nms_batch_case()
    n = tc.BATCH_COUNTS[2]
    _margin_and_share(bc.boxes[2, :n], bc.scores[2, :n], bc.labels[2, :n], bc.thr, bc.keep[2], 'batch sample 2')
    assert bc.keep[0].numel() == 0 and bc.keep[1].tolist() == [True]
    c = tc.nms_nan_case()
    f = c.finite
    _margin_and_share(c.boxes[f], c.scores[f], c.labels[f], c.thr, c.keep_finite, 'nan_scores, finite subset')
    assert bool(torch.isnan(c.scores[list(tc.NAN_AT)]).all()) and f.numel() == 37
    # the NaN-scored boxes overlap finite ones of their class: a kernel that let them suppress, or be ranked by a false comparison, would differ
    ious = tc.same_class_ious(c.boxes.numpy(), c.labels.numpy())
    assert sum(1 for (i, j), v in ious.items() if (i in tc.NAN_AT) != (j in tc.NAN_AT) and v > c.thr) >= 3
