"""Edge problems for the last four kernels of a frame -- decode_topk_kernel / decode_rank_emit, result_pack_kernel and pack_detections_kernel
of csrc/geometry.hip, nms_bev_kernel of csrc/nms.hip -- and their expected results, all computed on the CPU.  No tests here:
tests/test_tail_cases_cpu.py shows that the cases tell a correct kernel from one with a defect and pins the references below to
oracle/mv2d_oracle.py, tests/test_gpu_tail_edges.py holds the kernels to them.

Decode.  `decode_ranked` states the kernel's documented order: the flat candidates ranked by the monotone integer image of the logit BITS,
descending, lower flat index first among equals (torch.topk leaves the order of equal scores open, and sigmoid maps neighbouring logits to
one score); then the box code, the centre-range filter and z -= h / 2 exactly as O.decode applies them.  Where the selected scores are
distinct this IS O.decode (asserted on the CPU).  The cases sit on the edges of the kernel: n = R * N around max_num, around the 1024 slots
of the survivor array and around the 16384 keys that fit in LDS, max_num at both ends of [1, 1024], and ties of every size at the K-th rank
-- every key whose logit equals the K-th survives the radix select of the logit bits, so a plateau of equal logits (or of one NaN pattern)
overflows the survivor array.

Pack / wire / NMS: expectations are O.post_nms_pack, mv2d_amd.dist.pack_detections_batch and O.nms_bev.  The rows behind `count` of every
input hold GARBAGE (NaN boxes, score 2, label 10^6), which must not leak.  The random NMS cases are built so that no same-class pair has an
fp64 IoU within IOU_MARGIN of the threshold (one box of such a pair is deleted): |coordinates| <= 25 m at fp32 precision put a corner off
by about 3e-6 m, an area by about 5e-5 m^2 over unions >= 2.25 m^2, an IoU by about 3e-5; the margin is 3 x that."""
import functools
import math
import types

import numpy as np
import torch

from mv2d_amd import dist as mdist
from oracle import mv2d_oracle as O

NS = types.SimpleNamespace
POST = torch.tensor(O.POST_RANGE, dtype=torch.float32)
GARBAGE_SCORE, GARBAGE_LABEL = 2.0, 10 ** 6
IOU_MARGIN = 1e-4


# ------------------------------------------------------------------------------------------------ decode
def key_image(cls):
    """monotone uint32 image of the fp32 logit bits (the upper half of the kernel's key), flat"""
    u = cls.detach().contiguous().view(-1).numpy().view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def rank_flat(cls, max_num):
    """flat indices of the min(max_num, n) selected candidates in rank order"""
    img = key_image(cls).astype(np.int64)
    return torch.from_numpy(np.argsort(-img, kind='stable')[:min(max_num, img.size)].copy())


def emit(cls, reg, idx, num_classes, ge=torch.ge, le=torch.le):
    """O.decode from the ranked flat indices on (fp32 torch): boxes [m,9], scores, labels, bbox_index of the candidates inside the range
    (ge / le: the two comparisons of the range test, for the variants of tests/test_tail_cases_cpu.py)"""
    scores = cls.sigmoid().view(-1)[idx]
    labels, bbox_index = idx % num_classes, idx // num_classes
    bp = reg[bbox_index]
    rot = torch.atan2(bp[..., 6:7], bp[..., 7:8])
    boxes = torch.cat([bp[..., 0:1], bp[..., 1:2], bp[..., 4:5], bp[..., 2:3].exp(), bp[..., 3:4].exp(), bp[..., 5:6].exp(), rot, bp[:, 8:9],
                       bp[:, 9:10]], -1)
    rng = torch.tensor(O.POST_RANGE)
    mask = ge(boxes[..., :3], rng[:3]).all(1) & le(boxes[..., :3], rng[3:]).all(1)
    boxes, scores, labels, bbox_index = boxes[mask], scores[mask], labels[mask], bbox_index[mask]
    boxes = boxes.clone()
    boxes[:, 2] = boxes[:, 2] - boxes[:, 5] * 0.5
    return boxes, scores, labels, bbox_index


def decode_ranked(cls, reg, max_num, num_classes):
    return emit(cls, reg, rank_flat(cls, max_num), num_classes)


def _gen(seed):
    return np.random.Generator(np.random.PCG64(seed))


def distinct_logits(n, seed, lo=-6.0, hi=2.0):
    """n distinct fp32 logits (a shuffled ramp: no two equal, and the sigmoids of the largest ones distinct too)"""
    v = (lo + (hi - lo) * (_gen(seed).permutation(n).astype(np.float64) + 0.5) / n).astype(np.float32)
    assert np.unique(v).size == n
    return v


def make_reg(R, seed, spread=40.0):
    """bbox_preds [R,10]; spread 40: some centres outside POST_RANGE, spread <= 1: none"""
    reg = _gen(seed).standard_normal((R, 10)).astype(np.float32)
    reg[:, 0] *= spread; reg[:, 1] *= spread; reg[:, 4] *= spread * 0.15
    return reg


def _decode_case(name, R, N, max_num, logits, seed, spread=40.0, tie=False, reg=None):
    cls = torch.from_numpy(np.asarray(logits, dtype=np.float32).reshape(R, N).copy())
    reg = torch.from_numpy(make_reg(R, seed + 1, spread) if reg is None else reg)
    return NS(name=name, R=R, N=N, n=R * N, max_num=max_num, cls=cls, reg=reg, tie=tie)


# name -> (R, N, max_num): distinct logits, sizes on the edges of the kernel
DECODE_SIZES = {
    'n1': (1, 1, 300), 'n70': (7, 10, 300), 'n300': (30, 10, 300), 'n301': (43, 7, 300),           # around max_num
    'n1024': (128, 8, 300), 'n1025': (205, 5, 300),                                               # around the survivor array
    'n16384_lds': (256, 64, 300), 'n16385_stream': (16385, 1, 300),                               # the LDS / streamed split
    'k1': (30, 10, 1), 'k1024_n1024': (128, 8, 1024), 'k1024_n1280': (128, 10, 1024),             # max_num at its limits
}
DECODE_TIES = ('mass_tie_lds', 'boundary_tie', 'partial_tie', 'mass_tie_stream', 'nan_group', 'adjacent_floats', 'sign_and_specials')
DECODE_RANGE = ('range_edges', 'range_all_dropped', 'range_none_dropped')
DECODE_CASES = tuple(DECODE_SIZES) + DECODE_TIES + DECODE_RANGE
MASS_STREAM_TOP = (0, 4097, 9000, 15000, 300 * 64 - 1)           # flat indices of the 5 larger logits of mass_tie_stream
NAN_BITS = 0x7fc00000
SPECIALS = (np.inf, 3.4028235e38, 5.0, 1.1754944e-38, 1.1754942e-38, 1e-45, 0.0, -0.0, -1e-45, -1.1754942e-38, -1.1754944e-38, -5.0,
            -3.4028235e38, -np.inf)                                # ±inf, largest / smallest normals, subnormals, ±0 (fp32)
RANGE_ROWS = 30


def _range_reg(seed):
    """RANGE_ROWS rows inside the range; rows 2 + 2 k / 3 + 2 k (k = 0 .. 5) have one centre coordinate exactly ON bound k / one ulp outside"""
    reg = make_reg(RANGE_ROWS, seed, 0.5)
    col = (0, 1, 4, 0, 1, 4)
    on, off = [], []
    for k in range(6):
        b = np.float32(O.POST_RANGE[k])
        reg[2 + 2 * k, col[k]] = b
        reg[3 + 2 * k, col[k]] = np.nextafter(b, np.float32(-np.inf if k < 3 else np.inf), dtype=np.float32)
        on.append(2 + 2 * k); off.append(3 + 2 * k)
    return reg, on, off


@functools.lru_cache(maxsize=None)
def decode_case(name, seed=5100):
    if name in DECODE_SIZES:
        R, N, K = DECODE_SIZES[name]
        return _decode_case(name, R, N, K, distinct_logits(R * N, seed), seed)
    if name == 'mass_tie_lds':
        return _decode_case(name, 150, 10, 300, np.full(1500, -2.0), seed, spread=0.5, tie=True)
    if name == 'boundary_tie':                                    # the 1024th and 1025th largest equal: 1025 survivors at max_num = 1024
        v = distinct_logits(1280, seed)
        order = np.argsort(-v, kind='stable')
        v[order[1024]] = v[order[1023]]
        c = _decode_case(name, 128, 10, 1024, v, seed, spread=0.5, tie=True)
        c.pair = (int(order[1023]), int(order[1024]))
        return c
    if name == 'partial_tie':                                     # 100 distinct above a plateau of 2000, 900 distinct below
        g = _gen(seed)
        pos = g.permutation(3000)
        v = np.empty(3000, np.float32)
        v[pos[:100]] = distinct_logits(100, seed + 2, 1.0, 3.0)
        v[pos[100:2100]] = 0.5
        v[pos[2100:]] = distinct_logits(900, seed + 3, -6.0, 0.0)
        c = _decode_case(name, 300, 10, 300, v, seed, spread=0.5, tie=True)
        c.plateau = np.sort(pos[100:2100])
        return c
    if name == 'mass_tie_stream':
        v = np.full(300 * 64, -1.5, np.float32)
        v[list(MASS_STREAM_TOP)] = [0.25, 1.0, 0.5, 0.75, 2.0]
        return _decode_case(name, 300, 64, 300, v, seed, spread=0.5, tie=True)
    if name == 'nan_group':                                       # 1200 of one NaN pattern (the largest keys), 300 finite
        g = _gen(seed)
        pos = g.permutation(1500)
        u = distinct_logits(1500, seed).view(np.uint32).copy()
        u[pos[:1200]] = NAN_BITS
        c = _decode_case(name, 150, 10, 300, u.view(np.float32), seed, spread=0.5, tie=True)
        c.nan_idx = np.sort(pos[:1200])
        return c
    if name == 'adjacent_floats':                                 # 8 consecutive fp32 values around 1 and around -1
        g = _gen(seed)
        ladder = []
        for centre in (1.0, -1.0):
            x = np.float32(centre)
            for _ in range(4):
                x = np.nextafter(x, np.float32(-np.inf), dtype=np.float32)
            for _ in range(8):
                ladder.append(x)
                x = np.nextafter(x, np.float32(np.inf), dtype=np.float32)
        v = np.asarray(ladder, np.float32)[g.integers(0, 16, 400)]
        return _decode_case(name, 40, 10, 300, v, seed, spread=0.5, tie=True)
    if name == 'sign_and_specials':                               # every special twice + 4 ordinary values; max_num cuts between sigmoid groups
        g = _gen(seed)
        v = np.asarray(list(SPECIALS) * 2 + [1.0, -1.0, 2.0, -2.0], np.float32)[g.permutation(32)]
        K = int((v >= np.float32(-1.1754944e-38)).sum())          # down to -(smallest normal): sigmoid >= 0.5 of fp32
        return _decode_case(name, 16, 2, K, v, seed, spread=0.5, tie=True)
    if name == 'range_edges':
        reg, on, off = _range_reg(seed)
        c = _decode_case(name, RANGE_ROWS, 10, 300, distinct_logits(300, seed), seed, reg=reg)
        c.on, c.off = on, off
        return c
    if name == 'range_all_dropped':
        reg = make_reg(RANGE_ROWS, seed, 0.5)
        reg[:, 0] = np.nextafter(np.float32(O.POST_RANGE[3]), np.float32(np.inf), dtype=np.float32)
        return _decode_case(name, RANGE_ROWS, 10, 300, distinct_logits(300, seed), seed, reg=reg)
    if name == 'range_none_dropped':
        return _decode_case(name, RANGE_ROWS, 10, 300, distinct_logits(300, seed), seed, spread=0.5)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def decode_expected(name):
    c = decode_case(name)
    return decode_ranked(c.cls, c.reg, c.max_num, c.N)


GROUP_ROWS, GROUP_N, GROUP_MAX_NUM = (1, 0, 130, 103), 10, 300


@functools.lru_cache(maxsize=None)
def group_case(seed=5200):
    """one grouped launch: n < max_num, an empty sample, n > max_num with distinct logits, and a mass tie of 1030 equal logits"""
    start = np.concatenate([[0], np.cumsum(GROUP_ROWS)]).astype(np.int32)
    R = int(start[-1])
    v = distinct_logits(R * GROUP_N, seed)
    v[start[3] * GROUP_N:] = -0.75
    cls = torch.from_numpy(v.reshape(R, GROUP_N).copy())
    reg = torch.from_numpy(make_reg(R, seed + 1, 30.0))
    exp = [decode_ranked(cls[a:b], reg[a:b], GROUP_MAX_NUM, GROUP_N) for a, b in zip(start[:-1], start[1:])]
    return NS(R=R, N=GROUP_N, max_num=GROUP_MAX_NUM, cls=cls, reg=reg, grp_start=torch.from_numpy(start), max_grp_rows=max(GROUP_ROWS),
              expected=exp)


# ------------------------------------------------------------------------------------------------ pack
def _padded(boxes, scores, labels, count, stride):
    """rows [count, stride) hold garbage that must never be read"""
    b = torch.full((stride, 9), float('nan'))
    s = torch.full((stride,), GARBAGE_SCORE)
    l_ = torch.full((stride,), GARBAGE_LABEL, dtype=torch.int64)
    b[:count], s[:count], l_[:count] = boxes[:count], scores[:count], labels[:count]
    return b, s, l_


def _pack_case(name, count, stride, max_num, num_classes, seed, score_thr=0.0, scores=None, labels=None):
    g = _gen(seed)
    boxes = torch.from_numpy(g.standard_normal((count, 9)).astype(np.float32))
    if scores is None:
        scores = (g.permutation(count).astype(np.float32) + 1.0) / np.float32(count + 1)        # distinct, in (0, 1)
    if labels is None:
        labels = g.integers(0, num_classes, count)
    scores = torch.from_numpy(np.asarray(scores, np.float32))
    labels = torch.from_numpy(np.asarray(labels, np.int64))
    b, s, l_ = _padded(boxes, scores, labels, count, stride)
    return NS(name=name, count=count, stride=stride, max_num=max_num, num_classes=num_classes, score_thr=float(np.float32(score_thr)), boxes=b,
              scores=s, labels=l_)


PACK_CASES = ('count0', 'count1', 'count1024', 'survivors_eq_max', 'survivors_max_plus1', 'ones_fit', 'ones_over', 'ones_one_class_over',
              'thr_equal', 'nan_inf', 'one_class')
THR = np.float32(0.3)


@functools.lru_cache(maxsize=None)
def pack_case(name, seed=5300):
    g = _gen(seed + 7)
    if name == 'count0':
        return _pack_case(name, 0, 300, 300, 10, seed)
    if name == 'count1':
        return _pack_case(name, 1, 300, 300, 10, seed)
    if name == 'count1024':                                       # in_stride = max_num = 1024, labels up to 63
        lab = g.integers(0, 64, 1024); lab[[0, 500, 1023]] = 63
        return _pack_case(name, 1024, 1024, 1024, 64, seed, labels=lab)
    if name in ('survivors_eq_max', 'survivors_max_plus1'):       # 300 / 301 scores above score_thr: class-major, then global score order
        m = 300 if name == 'survivors_eq_max' else 301
        sc = (g.permutation(350).astype(np.float32) + 1.0) / np.float32(351)
        order = np.argsort(-sc)
        sc[order[m:]] *= np.float32(-1.0)                         # the rest not above score_thr = 0
        return _pack_case(name, 350, 400, 300, 10, seed, scores=sc)
    if name == 'ones_fit':                                        # saturated sigmoids: every score 1.0
        return _pack_case(name, 200, 300, 300, 10, seed, scores=np.ones(200))
    if name == 'ones_over':
        return _pack_case(name, 320, 320, 300, 10, seed, scores=np.ones(320))
    if name == 'ones_one_class_over':
        return _pack_case(name, 320, 400, 300, 10, seed, scores=np.ones(320), labels=np.full(320, 7))
    if name == 'thr_equal':                                       # scores equal to score_thr bit for bit are dropped (strict >)
        sc = (g.permutation(120).astype(np.float32) + 1.0) / np.float32(121)
        sc[[3, 50, 119]] = THR
        sc[[4, 51]] = np.nextafter(THR, np.float32(1), dtype=np.float32)
        sc[[5, 52]] = np.nextafter(THR, np.float32(0), dtype=np.float32)
        c = _pack_case(name, 120, 300, 300, 10, seed, score_thr=THR, scores=sc)
        c.at_thr = [3, 50, 119]
        return c
    if name == 'nan_inf':                                         # what the NMS stage hands over: -inf (suppressed) and NaN scores
        sc = (g.permutation(150).astype(np.float32) + 1.0) / np.float32(151)
        sc[[0, 7, 70, 149]] = np.nan
        sc[[1, 8, 71, 148]] = -np.inf
        return _pack_case(name, 150, 300, 100, 10, seed, scores=sc)
    if name == 'one_class':
        return _pack_case(name, 280, 300, 300, 10, seed, labels=np.full(280, 3))
    raise KeyError(name)


def pack_expected(c):
    n = c.count
    return O.post_nms_pack(c.boxes[:n], c.scores[:n], c.labels[:n], num_classes=c.num_classes, score_thr=c.score_thr, max_num=c.max_num)


BATCH_COUNTS, BATCH_STRIDE = (0, 1, 260), 300


@functools.lru_cache(maxsize=None)
def pack_batch_case(seed=5400):
    """3 samples at in_stride 300 with counts (0, 1, 260): boxes [3,300,9], scores, labels, count"""
    cs = [_pack_case('batch%d' % b, n, BATCH_STRIDE, 300, 10, seed + b) for b, n in enumerate(BATCH_COUNTS)]
    return NS(samples=cs, boxes=torch.stack([c.boxes for c in cs]), scores=torch.stack([c.scores for c in cs]),
              labels=torch.stack([c.labels for c in cs]), count=torch.tensor(BATCH_COUNTS, dtype=torch.int32), max_num=300, score_thr=0.0)


# ------------------------------------------------------------------------------------------------ wire
WIRE_MAX_NUM, WIRE_STRIDE = 100, 128
WIRE_COUNTS = (0, 1, WIRE_MAX_NUM, 37, WIRE_MAX_NUM + 7)          # the last: count > max_num at in_stride > max_num (the count goes out unclamped)


@functools.lru_cache(maxsize=None)
def wire_case(seed=5500):
    cs = []
    for b, n in enumerate(WIRE_COUNTS):
        lab = _gen(seed + 50 + b).integers(0, 64, n)
        lab[:1] = 63
        cs.append(_pack_case('wire%d' % b, n, WIRE_STRIDE, WIRE_MAX_NUM, 64, seed + b, labels=lab))
    c = NS(boxes=torch.stack([c.boxes for c in cs]), scores=torch.stack([c.scores for c in cs]), labels=torch.stack([c.labels for c in cs]),
           count=torch.tensor(WIRE_COUNTS, dtype=torch.int32), max_num=WIRE_MAX_NUM, stride=WIRE_STRIDE)
    c.expected = mdist.pack_detections_batch(c.boxes, c.scores, c.labels, c.count, WIRE_MAX_NUM)
    return c


# ------------------------------------------------------------------------------------------------ NMS
def _box(x, y, dx, dy, yaw=0.0):
    return [x, y, 0.0, dx, dy, 1.5, yaw, 0.0, 0.0]


def _nms_case(name, boxes, scores, labels, thr, random=False):
    boxes = torch.tensor(np.asarray(boxes, np.float32).reshape(-1, 9))
    return NS(name=name, n=boxes.shape[0], boxes=boxes, scores=torch.tensor(np.asarray(scores, np.float32).reshape(-1)),
              labels=torch.tensor(np.asarray(labels, np.int64).reshape(-1)), thr=float(thr), random=random)


def same_class_ious(boxes, labels):
    """{(i, j): fp64 IoU} of the same-class pairs i < j whose bounding circles meet (every other pair is disjoint: IoU 0)"""
    b = np.asarray(boxes, np.float64)
    rad = 0.5 * np.hypot(b[:, 3], b[:, 4])
    out = {}
    for c in np.unique(labels):
        ids = np.nonzero(np.asarray(labels) == c)[0]
        for a_, i in enumerate(ids):
            rest = ids[a_ + 1:]
            near = rest[np.hypot(b[rest, 0] - b[i, 0], b[rest, 1] - b[i, 1]) <= rad[rest] + rad[i]]
            for j in near:
                out[(int(i), int(j))] = O.rotated_iou_bev(b[i], b[j])
    return out


def _random_boxes(n, n_classes, n_clusters, thr, seed, sigma=0.8):
    """seeded clustered boxes; one box (the higher index) of every same-class pair whose IoU is within IOU_MARGIN of thr is deleted"""
    g = _gen(seed)
    centres = g.random((n_clusters, 2)) * 40 - 20
    extra = n // 16 + 4
    m = n + extra
    boxes = np.zeros((m, 9), np.float32)
    boxes[:, :2] = centres[g.integers(0, n_clusters, m)] + g.normal(0, sigma, (m, 2))
    boxes[:, 3:5] = g.random((m, 2)) * 3 + 1.5
    boxes[:, 5] = 1.5
    boxes[:, 6] = g.random(m) * 2 * math.pi - math.pi
    scores = ((g.permutation(m).astype(np.float32) + 1.0) / np.float32(m + 1))
    labels = g.integers(0, n_classes, m)
    drop = sorted({j for (i, j), v in same_class_ious(boxes, labels).items() if abs(v - thr) < IOU_MARGIN})
    assert len(drop) <= extra, 'more close pairs than spare boxes'
    keep = np.setdiff1d(np.arange(m), drop)[:n]
    return boxes[keep], scores[keep], labels[keep]


# closed forms of test_rotated_bev_nms_below_threshold_one: (box a, box b, IoU)
_OCT = 2 * (math.sqrt(2) - 1)
CLOSED_FORMS = (
    ('shift_half', _box(0, 0, 1, 1), _box(0.5, 0, 1, 1), 1 / 3),
    ('turn_90', _box(0, 0, 2, 1), _box(0, 0, 2, 1, math.pi / 2), 1 / 3),
    ('octagon', _box(0, 0, 1, 1), _box(0, 0, 1, 1, math.pi / 4), _OCT / (2 - _OCT)),
)
NMS_RANDOM = ('big1024', 'rand260')
NMS_CASES = (('n0', 'n1', 'n2', 'identical', 'nested_in', 'nested_out', 'touching', 'zero_area', 'yaws', 'chain', 'cross_class', 'score_ties',
              'thr_one') + tuple('%s_%s' % (n, s) for n, _, _, _ in CLOSED_FORMS for s in ('below', 'above')) + NMS_RANDOM)


@functools.lru_cache(maxsize=None)
def nms_case(name, seed=5600):
    if name == 'n0':
        return _nms_case(name, np.zeros((0, 9)), [], [], 0.3)
    if name == 'n1':
        return _nms_case(name, [_box(1, 2, 3, 2, 0.4)], [0.5], [2], 0.3)
    if name == 'n2':                                              # the second, higher-scored box suppresses the first
        return _nms_case(name, [_box(0, 0, 2, 2), _box(0.25, 0, 2, 2)], [0.4, 0.6], [1, 1], 0.3)
    if name == 'identical':                                       # copies: the best score survives, the lower index among equal scores
        b = [_box(3, -2, 2, 1, 0.3)] * 4 + [_box(-8, 5, 1.5, 3, -1.0)] * 3
        return _nms_case(name, b, [0.5, 0.9, 0.9, 0.2, 0.7, 0.7, 0.7], [0] * 7, 0.5)
    if name in ('nested_in', 'nested_out'):                       # 1 x 1 inside 2 x 2: IoU 1/4
        return _nms_case(name, [_box(0, 0, 2, 2), _box(0.25, 0.25, 1, 1)], [0.9, 0.8], [0, 0], 0.2 if name == 'nested_in' else 0.3)
    if name == 'touching':                                        # a shared edge, a shared corner, disjoint: IoU 0 exactly (integer corners), thr 0
        b = [_box(0, 0, 2, 2), _box(2, 0, 2, 2), _box(2, 2, 2, 2), _box(-2, -2, 2, 2), _box(10, 10, 2, 2)]
        return _nms_case(name, b, [0.9, 0.8, 0.7, 0.6, 0.5], [0] * 5, 0.0)
    if name == 'zero_area':                                       # degenerate boxes suppress nothing and are not suppressed
        b = [_box(0, 0, 2, 2), _box(0, 0, 0, 2), _box(0, 0, 0, 2), _box(0.5, 0, 2, 0), _box(0, 0, 0, 0), _box(0.25, 0, 2, 2)]
        return _nms_case(name, b, [0.9, 0.8, 0.7, 0.6, 0.5, 0.4], [0] * 6, 0.1)
    if name == 'yaws':                                            # 2 x 1 at yaw 0 / ±pi/2 / ±pi about one centre: IoU 1 or 1/3
        b = [_box(0, 0, 2, 1, y) for y in (0.0, math.pi, -math.pi, math.pi / 2, -math.pi / 2)] + [_box(9, 9, 2, 1, math.pi / 2), _box(9, 9, 2, 1, 0.0)]
        return _nms_case(name, b, [0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3], [0] * 7, 0.5)
    if name == 'chain':                                           # A kills B (IoU 0.6); B would kill C (0.6); A and C: 1/3 -> C stays
        return _nms_case(name, [_box(1.0, 0, 2, 1), _box(0.5, 0, 2, 1), _box(0, 0, 2, 1)], [0.7, 0.8, 0.9], [4, 4, 4], 0.5)
    if name == 'cross_class':                                     # heavy overlap across classes does not suppress
        return _nms_case(name, [_box(0, 0, 2, 2, 0.1), _box(0.1, 0, 2, 2, 0.1), _box(0, 0.1, 2, 2, 0.1), _box(0.1, 0.1, 2, 2, 0.1)],
                         [0.9, 0.8, 0.7, 0.6], [0, 1, 2, 0], 0.3)
    if name == 'score_ties':                                      # equal scores: the lower index goes first
        b = [_box(0.3 * i, 0, 2, 2, 0.2) for i in range(6)]
        return _nms_case(name, b, [0.5] * 6, [1] * 6, 0.5)
    if name == 'thr_one':                                         # IoU == 1.0f == thr: strict >, nothing suppressed
        return _nms_case(name, [_box(1, 1, 2, 4)] * 3, [0.5, 0.6, 0.7], [0] * 3, 1.0)
    for cf, a, b, iou in CLOSED_FORMS:
        if name == cf + '_below':
            return _nms_case(name, [a, b], [0.9, 0.8], [0, 0], iou - 1e-3)
        if name == cf + '_above':
            return _nms_case(name, [a, b], [0.9, 0.8], [0, 0], iou + 1e-3)
    if name == 'big1024':                                         # in_stride = n = 1024
        return _nms_case(name, *_random_boxes(1024, 16, 80, 0.2, seed, sigma=0.8), 0.2, random=True)
    if name == 'rand260':
        return _nms_case(name, *_random_boxes(260, 4, 20, 0.2, seed + 1), 0.2, random=True)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def nms_expected(name):
    c = nms_case(name)
    return torch.from_numpy(O.nms_bev(c.boxes.numpy(), c.scores.numpy(), c.labels.numpy(), c.thr).astype(bool))


NMS_BATCH_THR = 0.2


@functools.lru_cache(maxsize=None)
def nms_batch_case(seed=5700):
    """the layout of pack_batch_case -- counts (0, 1, 260) at in_stride 300, garbage behind -- with clustered boxes; expected keep per sample"""
    cs = []
    for b, n in enumerate(BATCH_COUNTS):
        bx, sc, lb = _random_boxes(n, 4, 20, NMS_BATCH_THR, seed + b) if n > 1 else (np.asarray([_box(1, 1, 2, 3, 0.5)] * n, np.float32).reshape(n, 9),
                                                                                      np.full(n, 0.5, np.float32), np.zeros(n, np.int64))
        cs.append(_padded(torch.from_numpy(bx), torch.from_numpy(sc), torch.from_numpy(lb), n, BATCH_STRIDE))
    keep = [torch.from_numpy(O.nms_bev(b[:n].numpy(), s[:n].numpy(), l_[:n].numpy(), NMS_BATCH_THR).astype(bool))
            for (b, s, l_), n in zip(cs, BATCH_COUNTS)]
    return NS(boxes=torch.stack([c[0] for c in cs]), scores=torch.stack([c[1] for c in cs]), labels=torch.stack([c[2] for c in cs]),
              count=torch.tensor(BATCH_COUNTS, dtype=torch.int32), thr=NMS_BATCH_THR, keep=keep, max_num=300)


NAN_AT = (0, 17, 39)


@functools.lru_cache(maxsize=None)
def nms_nan_case(seed=5800):
    """40 boxes, three of them with NaN scores: those take no part; the other 37 are O.nms_bev of the finite subset"""
    bx, sc, lb = _random_boxes(40, 2, 4, 0.2, seed)
    sc = sc.copy()
    sc[list(NAN_AT)] = np.nan
    fin = np.setdiff1d(np.arange(40), NAN_AT)
    keep = O.nms_bev(bx[fin], sc[fin], lb[fin], 0.2).astype(bool)
    c = _nms_case('nan_scores', bx, sc, lb, 0.2)
    c.finite, c.keep_finite = torch.from_numpy(fin), torch.from_numpy(keep)
    return c
