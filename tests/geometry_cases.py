"""Edge problems for the frame-geometry kernels of csrc/geometry.hip (box_params_row, box_corr_block, frame_geometry_kernel, the T-path
mask / compaction / CSR chain and the S-path CSR) and their expected results from oracle/mv2d_oracle.py.  No tests here:
tests/test_geometry_cases_cpu.py shows on the CPU that the cases tell a correct kernel from one with a defect, tests/test_gpu_geometry_edges.py
holds the kernels to them.

The rig is the overlapping one of the `nc6_s` workload cut to 3 views (yaw step 8 degrees, baseline 0.35 m, image 224 x 400 padded to 416
columns: a 14 x 26 map whose last column is padding), so that RoIs of different views are matched with each other.  A case is a layout of
per-view RoI counts (LAYOUTS) filled with seeded boxes 6 .. 150 px wide and 6 .. 120 px high (some of them cross the right image border) and,
in every view with at least SPECIAL_MIN boxes, the boxes of SPECIAL at the indices 2 ..: narrower / lower than 4 px, exactly 4 and exactly
16 px (`small` tests with a strict <), below one map cell, a quarter pixel wide (intr_scale = 1 then exceeds the 5e3 clamp at f = 320 px),
touching, crossing and wholly outside the image, and in the padded column only; behind them `tight`, a box that equals the epipolar
rectangle of a box of another view bit for bit (IoU == 1.0f: the one value at which `>` and `>=` against iou_thr = 1 part).  Exact duplicates: in a view with more than DUP_OFFSET
boxes the boxes DUP_OFFSET + j copy the boxes j (up to DUP_MAX of them: twins more than 128 indices apart, the stride of the kernel's
IoU and rank loops); every other view with at least SPECIAL_MIN boxes ends with a copy of its first box.  The twins' IoUs with any
rectangle are equal bit for bit, so their order in a top-k list is the tie rule's alone, and with DUP_MAX odd and distinct boxes behind
them the tied pairs fall on both parities of the rank.

`batch` is a two-sample launch (2 x 3 views, view ids 0 .. 5, the second sample on a rig of its own) laid out as the engine lays a batch out:
trans [6][3][16], the per-view tables and the padding mask of the samples one after the other."""
import functools
import types

import numpy as np
import torch

from mv2d_amd import calib, synthetic
from oracle import mv2d_oracle as O

VIEWS, IMG_H, IMG_W, PAD_W, STRIDE = 3, 224, 400, 416, 16
MAP_H, MAP_W = IMG_H // STRIDE, PAD_W // STRIDE
FOCAL = 0.8 * IMG_W
SPECIAL_MIN, DUP_OFFSET, DUP_MAX = 30, 130, 65

# name -> per-view counts (a tuple of tuples: one entry per sample)
LAYOUTS = {
    'mid_empty': ((260, 0, 131),),            # one view of >= 257 RoIs, an empty one in the middle, one of >= 129
    'first_empty': ((0, 140, 60),),
    'last_empty': ((150, 40, 0),),
    'r1': ((0, 1, 0),),
    'r127': ((50, 40, 37),),                  # R = 127, 128, 129: the edges of the ceil(R / 128) camera blocks of frame_geometry_kernel
    'r128': ((43, 0, 85),),
    'r129': ((60, 29, 40),),
    'batch': ((40, 0, 33), (31, 36, 0)),
}
SINGLE = tuple(n for n, l in LAYOUTS.items() if len(l) == 1)
RIGS = ((8.0, 0.35), (10.0, 0.3))             # (yaw step in degrees, baseline in metres) of sample 0, 1

SPECIAL = (
    ('w3', (100.0, 60.0, 103.0, 100.0)),          # narrower than min_size = 4
    ('h3', (150.0, 60.0, 190.0, 63.0)),           # lower than 4, wide enough: a test of the width alone misses it
    ('w4', (100.0, 110.0, 104.0, 150.0)),         # exactly 4: not small
    ('h4', (150.0, 110.0, 190.0, 114.0)),
    ('w16', (200.0, 60.0, 216.0, 100.0)),         # exactly 16: not small under min_size = 16
    ('h16', (230.0, 60.0, 270.0, 76.0)),
    ('w15', (200.0, 120.0, 215.0, 160.0)),
    ('sub_cell', (300.5, 100.5, 302.0, 102.5)),   # below one 16 px cell
    ('clamp', (120.0, 130.0, 120.25, 170.0)),     # fx * 7 / 0.25 = 8960 > 5e3
    ('touch_tl', (0.0, 0.0, 50.0, 40.0)),
    ('touch_br', (340.0, 180.0, 399.0, 223.0)),
    ('cross_l', (-20.0, 50.0, 30.0, 100.0)),
    ('cross_r', (380.0, 90.0, 430.0, 150.0)),     # over the image border and the padded one
    ('cross_t', (60.0, -30.0, 120.0, 25.0)),
    ('cross_b', (60.0, 200.0, 130.0, 260.0)),
    ('out_left', (-200.0, 40.0, -120.0, 100.0)),  # wholly outside, more than expand_stride = 2 cells away
    ('out_below', (100.0, 300.0, 180.0, 380.0)),  # ... and no projected sample can be valid: an empty CSR row
    ('pad_col', (401.0, 80.0, 415.0, 140.0)),     # the padded column only
)
SMALL_4 = ('w3', 'h3', 'sub_cell', 'clamp')       # zeroed by min_size = 4
TIGHT = 2 + len(SPECIAL)                          # index of the `tight` box in its view (see _sample)

# (sample_size, num_depth, depth_start, iou_thr, ratio, topk): a list, not a product; every value of the three groups
#   (sample_size, num_depth, depth_start) in (4, 8, 0.5), (3, 14, 0.5), (2, 32, 1.0), (5, 5, 0.25), (1, 8, 0.5)   [126, 128, 125, 8 samples]
#   (iou_thr, ratio) in (0, 0), (0.3, 0.5), (0.05, 2.0), (1.0, 1.0);  topk in 1, 5, 20, 300
# occurs.  depth_start is fp32-representable: the kernel takes it as float, the oracle compares in double.
PARAM_SETS = (
    (4, 8, 0.5, 0.0, 0.0, 20),
    (4, 8, 0.5, 0.3, 0.5, 5),
    (3, 14, 0.5, 0.05, 2.0, 1),
    (2, 32, 1.0, 0.3, 0.5, 300),
    (5, 5, 0.25, 0.05, 2.0, 20),
    (1, 8, 0.5, 0.0, 0.0, 5),
    (4, 8, 0.5, 1.0, 1.0, 20),
    (2, 32, 1.0, 0.0, 0.0, 1),
)
Params = types.SimpleNamespace


def params(ps):
    ss, D, ds, thr, ratio, topk = ps
    assert ss * ss * D <= 128 and float(np.float32(ds)) == ds
    return Params(sample_size=ss, num_depth=D, depth_start=ds, iou_thr=thr, ratio=ratio, topk=topk, key=ps)


def tables(p):
    """lin / depths of the parameter set, as the engine would build them"""
    return calib.constant_tables(p.sample_size, p.num_depth, p.depth_start)


def _epipolar_rect(box, a, b, metas):
    """bounding rectangle (x1, y1, x2, y2) fp32 of the valid samples of `box` (view a) in view b at the default sampling keys, exactly as
    epipolar_in_box builds it, or None without a valid sample"""
    roi = torch.tensor([[float(a)] + [float(x) for x in box]], dtype=torch.float32)
    uv, valid = O.epipolar_in_each_view(O.sample_points_in_rois(roi, 4).reshape(16, 3), metas[0]['pad_shape'], O.view_transforms(metas))
    uv, valid = uv[:, b].reshape(-1, 2), valid[:, b].reshape(-1)
    if not bool(valid.any()):
        return None
    return torch.cat([uv[valid].min(0)[0], uv[valid].max(0)[0]]).numpy()


def _sample(counts, seed, rig):
    metas = synthetic.make_img_metas(VIEWS, IMG_H, IMG_W, 1, pad_w=PAD_W, yaw_step_deg=rig[0], baseline=rig[1])
    props = synthetic.make_proposals(VIEWS, list(counts), IMG_H, IMG_W, seed, wh_lo=(6.0, 6.0), wh_hi=(150.0, 120.0))
    special, twins = {}, []
    full = [v for v, n in enumerate(counts) if n >= SPECIAL_MIN]
    for v in full:
        for j, (name, box) in enumerate(SPECIAL):
            props[v][2 + j, :4] = np.asarray(box, dtype=np.float32)
            special.setdefault(name, []).append((v, 2 + j))
    if len(full) >= 2:
        # `tight`: a box of view b that IS the epipolar rectangle of a box of view a (the first one whose rectangle is large enough that the
        # 1e-4 of the IoU's denominator vanishes in fp32): inter == union == area, IoU == 1.0f exactly == iou_thr of the (1, 1) parameter set
        a, b = full[0], full[1]
        for i in [0, 1] + list(range(TIGHT + 1, counts[a])):
            rect = _epipolar_rect(props[a][i, :4], a, b, metas)
            if rect is not None and (rect[2] - rect[0]) * (rect[3] - rect[1]) >= 4096.0:
                props[b][TIGHT, :4] = rect
                special['tight'] = [(b, TIGHT)]
                special['tight_source'] = [(a, i)]
                break
    for v in full:
        n = counts[v]
        if n > DUP_OFFSET:
            for j in range(min(n - DUP_OFFSET, DUP_MAX)):
                props[v][DUP_OFFSET + j, :4] = props[v][j, :4]
                twins.append((v, j, DUP_OFFSET + j))
        else:
            props[v][n - 1, :4] = props[v][0, :4]
            twins.append((v, 0, n - 1))
    return [torch.from_numpy(p) for p in props], metas, special, twins


@functools.lru_cache(maxsize=None)
def make_case(name, seed=4100):
    layout = LAYOUTS[name]
    B = len(layout)
    samples, rois, npv, special, twins = [], [], [], {}, []
    r0 = 0
    for b, counts in enumerate(layout):
        props, metas, sp, tw = _sample(counts, seed + 17 * b, RIGS[b])
        rl = O.bbox2roi(props)
        start = np.concatenate([[0], np.cumsum(counts)]).astype(int)
        for k, lst in sp.items():
            special.setdefault(k, []).extend(r0 + int(start[v]) + i for v, i in lst)
        twins += [(r0 + int(start[v]) + i, r0 + int(start[v]) + j) for v, i, j in tw]
        samples.append(types.SimpleNamespace(props=props, metas=metas, rois=rl, npv=list(counts), first=r0))
        rg = rl.clone()
        rg[:, 0] += b * VIEWS
        rois.append(rg)
        npv += list(counts)
        r0 += rl.shape[0]
    geo = [calib.geometry_tables(s.metas) for s in samples]
    shp = [calib.shape_tables(calib.meta_shapes(s.metas), MAP_H, MAP_W) for s in samples]
    return types.SimpleNamespace(
        name=name, B=B, V=VIEWS, h=MAP_H, w=MAP_W, samples=samples, rois=torch.cat(rois).contiguous(), R=r0, npv=npv,
        proposals=[p for s in samples for p in s.props], img_metas=[m for s in samples for m in s.metas],
        view_start=torch.tensor(np.concatenate([[0], np.cumsum(npv)]), dtype=torch.int32), max_per_view=max(npv),
        viewK=torch.cat([g['viewK'] for g in geo]).contiguous(), viewE=torch.cat([g['viewE'] for g in geo]).contiguous(),
        trans=torch.cat([g['trans'] for g in geo]).contiguous(),                       # [B * V][V][16]
        pad_mask=torch.cat([s_['pad_mask'] for s_ in shp]).contiguous(), pad_h=shp[0]['pad_h'], pad_w=shp[0]['pad_w'],
        special=special, twins=twins)


def view_of(case, ids):
    """global view index of global RoI ids"""
    return np.searchsorted(case.view_start.numpy(), np.asarray(ids), side='right') - 1


@functools.lru_cache(maxsize=None)
def epipolar(name, ps):
    """epipolar_in_box of every sample of the case: per RoI the list of (global RoI id, keep) in (view, IoU rank) order"""
    case, p = make_case(name), params(ps)
    out = []
    for s in case.samples:
        ep = O.epipolar_in_box(s.rois, s.npv, s.metas[0]['pad_shape'], O.view_transforms(s.metas), p.topk, p.iou_thr, p.ratio, p.sample_size,
                               p.num_depth, p.depth_start)
        out += [[(i + s.first, k) for i, k in row] for row in ep]
    return out


def match_from_lists(case, ep, topk):
    """(match [R, V, topk] int32, length [R, V]): position by position what mv2d_box_correlation writes -- the oracle's id where it keeps the
    entry, -1 where it does not, -1 behind the list, in the RoI's own view and in a view without RoIs."""
    match = np.full((case.R, case.V, topk), -1, dtype=np.int32)
    length = np.zeros((case.R, case.V), dtype=np.int64)
    for r, row in enumerate(ep):
        if not row:
            continue
        ids = np.asarray([i for i, _ in row], dtype=np.int32)
        keep = np.asarray([k for _, k in row], dtype=bool)
        vl = view_of(case, ids) % case.V
        assert (np.diff(vl) >= 0).all()
        for v in np.unique(vl):
            sel = vl == v
            n = int(sel.sum())
            match[r, v, :n] = np.where(keep[sel], ids[sel], -1)
            length[r, v] = n
    return torch.from_numpy(match), torch.from_numpy(length)


def expected_match(name, ps):
    return match_from_lists(make_case(name), epipolar(name, ps), ps[5])


def rows_skipping_gaps(match):
    """what a consumer of match lists per RoI: itself, then every entry >= 0 of its V * topk row in order"""
    return [[r] + [x for x in row if x >= 0] for r, row in enumerate(match.reshape(match.shape[0], -1).tolist())]


def box_params_ref(case, roi_size=7):
    """(K_roi [R,4,4] fp64, E [R,4,4] fp64) of get_box_params"""
    return O.get_box_params(case.proposals, [m['intrinsics'] for m in case.img_metas], [m['extrinsics'] for m in case.img_metas],
                            roi_size=(roi_size, roi_size))


def intr_ref(case, K_roi, intr_scale, min_size):
    return O.process_intrins_feat(case.rois, K_roi, intr_scale, min_size).clamp(-5e3, 5e3)


def t_path_ref(name, ps, expand):
    """(ffr [R,V,h,w] bool, pad [V,h,w] bool) of a single-sample case: gen_box_correlation and padding_mask"""
    case, p = make_case(name), params(ps)
    assert case.B == 1
    ffr = O.gen_box_correlation(case.rois, case.npv, case.img_metas, case.h, case.w, STRIDE, expand, p.topk, p.iou_thr, p.ratio, p.sample_size,
                                p.num_depth, p.depth_start)
    return ffr, O.padding_mask(case.img_metas, case.h, case.w)
