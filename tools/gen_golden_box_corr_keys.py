"""Reference goldens for box_correlation's sampling keys and intrins_feat_scale (build container only: needs the reference tree; never run on
the GPU machine).

    python -B tools/gen_golden_box_corr_keys.py [kernel] [e2e]     # writes tests/golden/box_corr_keys_kernel.npz, box_corr_keys_<case>.npz,
                                                                   # box_corr_keys_refnoise.npz and README_box_corr_keys.md

Kernel level: the UNMODIFIED reference ``BoxCorrelation(...).epipolar_in_box`` on the RoIs and matrices of ``geometry_cases.make_case('r127')`` and
``make_case('mid_empty')`` for every parameter set of KEY_SETS, stored in the ``match [R, V, topk]`` form of ``geometry_cases.match_from_lists``.
For every LID=True set ``oracle.mv2d_oracle.epipolar_in_box`` must give the same array, and on r127 every set must differ from the default keys
(same topk) for at least a quarter of the RoIs.

End to end: the reference MV2DSHead / MV2DTHead built from ``configs.roi_head_cfg_s / _t(box_correlation=..., intrins_feat_scale=...)`` on the
``corr3_s`` / ``corr3_t`` problems through ``oracle.gen_golden.run_case`` under every execution variant of ``oracle.gen_golden_refnoise.VARIANTS``:
the 't8' run is the golden, the others give the reference's own rank noise.  The match lists at the case's keys must differ from those of the same
head at the default keys, or the next problem seed is taken.  The files hold arrays only.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import geometry_cases as gc  # noqa: E402
from mv2d_amd import configs, ops, synthetic  # noqa: E402
from oracle import _stubs  # noqa: E402
from oracle import mv2d_oracle as O  # noqa: E402
from oracle.gen_golden import OUT, run_case  # noqa: E402
from oracle.gen_golden_refnoise import VARIANTS, ranked_diff  # noqa: E402

# (sample_size, num_depth, depth_start, depth_end, LID, topk)
KEY_SETS = (
    (2, 33, 0.5, 70, True, 20),        # 132 samples: one stride + 4
    (4, 16, 0.5, 70, True, 1),         # 256: two full strides
    (3, 29, 1.0, 50, True, 5),         # 261
    (8, 64, 0.5, 70, True, 20),        # 4096: the bound
    (4, 8, 0.5, 35, True, 20),         # 128, depth_end only
    (4, 8, 0.5, 70, False, 20),        # 128, uniform bins
    (6, 16, 0.3, 60, False, 300),      # 576
)
DEFAULT_KEYS = (4, 8, 0.5, 70, True)
KERNEL_CASES = ('r127', 'mid_empty')
E2E_KEYS = dict(sample_size=6, num_depth=16, depth_start=0.3, depth_end=60, LID=False)
# (case, problem, box_correlation keys, intrins_feat_scale)
E2E_CASES = (('corr3_s_keys', 'corr3_s', E2E_KEYS, 0.05),
             ('corr3_t_keys', 'corr3_t', E2E_KEYS, 0.05),
             ('corr3_s_scale', 'corr3_s', None, 0.25))
KEEP = ('intr', 'center_pred', 'xyz', 'feat_for_rois', 'feat_for_rois_shape', 'key_padding', 'corr', 'corr_mask', 'ref', 'cls', 'reg', 'boxes', 'scores',
        'labels', 'topk_index', 'topk_scores')
NOISE_MAX = 4
MAX_SEED = 8


def set_name(ks):
    return 'ss%d_d%d_%s_%s_%s_k%d' % (ks[0], ks[1], ks[2], ks[3], 'lid' if ks[4] else 'uni', ks[5])


TIES = {}          # (layout, keys, topk) -> (RoI, view) lists in which the reference's own order at bit-equal IoUs was not the canonical one


def reference_match(Ref, case, keys, topk):
    """match [R, V, topk] int32 of the reference's epipolar_in_box (one sample).  Per (RoI, matched view) the reference lists min(topk, max RoIs of
    a view) ids in IoU rank order with a keep mask; a kept id goes to its rank in its view's row, everything else is -1.

    Its argsort (box_correlation.py:370) is unstable, so RoIs whose IoUs with the epipolar rectangle are equal bit for bit (duplicate boxes, boxes of
    equal area inside the rectangle) come out in either order.  The golden holds such runs in the order of the RoI index, which is
    oracle.mv2d_oracle's and the kernel's tie rule: the IoUs the reference computed are read off its own box_iou call (wrapped for the run, as
    oracle.gen_golden.run_case wraps the heads' methods), and every list is checked to be the reference's up to the order inside runs of
    bit-equal IoUs -- the same keep mask, and at every kept rank the same IoU."""
    assert case.B == 1
    ss, D, ds, de, lid = keys
    mod = Ref(sample_size=ss, num_depth=D, depth_start=ds, depth_end=de, LID=lid, correlation_mode='topk_matched:%d:0.0:0.0' % topk)
    s = case.samples[0]
    seen_iou, orig = [], Ref.box_iou

    def spy(a, b, eps=1e-4):
        r = orig(a, b, eps)
        seen_iou.append((r[:, 0].clone(), b.clone()))
        return r
    Ref.box_iou = staticmethod(spy)
    try:
        corr, mask = mod.epipolar_in_box(s.rois, s.metas[0]['pad_shape'], O.view_transforms(s.metas), s.npv, s.metas)
    finally:
        Ref.box_iou = staticmethod(orig)
    (iou_rows, boxes_rows), = seen_iou                       # [rows, max RoIs], [rows, max RoIs, 4]: one row per (RoI, matched view), RoI-major
    corr, mask, iou_rows = corr.numpy(), mask.numpy(), iou_rows.numpy()
    pads = torch.nn.utils.rnn.pad_sequence(s.rois.split(s.npv, 0), batch_first=True)[..., 1:]
    row_view = [next(v for v in range(case.V) if s.npv[v] and torch.equal(pads[v], bx)) for bx in boxes_rows]
    start = case.view_start.numpy()
    w = min(topk, max(s.npv))
    assert corr.shape[1] % w == 0
    match = np.full((case.R, case.V, topk), -1, dtype=np.int32)
    i, ties = 0, []
    for r in range(case.R):
        for j in range(corr.shape[1] // w):
            ids, keep = corr[r, j * w:(j + 1) * w], mask[r, j * w:(j + 1) * w]
            if not keep.any() and not (ids != 0).any():
                # padding behind the RoI's last view -- or, at w = 1, the list of view 0 with RoI 0 on top at IoU 0: nothing is kept either way
                if j == 0 and w == 1 and i < len(row_view) and row_view[i] == 0 and not (iou_rows[i][:s.npv[0]] > 0).any():
                    i += 1
                break
            v = row_view[i]
            nb = s.npv[v]
            iou = iou_rows[i][:nb]
            i += 1
            order = np.argsort(-iou, kind='stable')[:w]
            can_keep = iou[order] > 0
            n = len(order)
            assert (keep[:n] == can_keep).all() and not keep[n:].any(), (r, v)
            assert (gc.view_of(case, ids[keep]) == v).all() and (iou[ids[:n][can_keep] - start[v]] == iou[order][can_keep]).all(), (r, v)
            if (ids[:n][can_keep] != order[can_keep] + start[v]).any():
                ties.append((r, v))
            match[r, v, :n] = np.where(can_keep, order + start[v], -1)
    assert i == len(row_view), (i, len(row_view))
    TIES[(case.name, keys, topk)] = ties
    return match


def kernel_level(Ref):
    store, lines = {}, []
    for name in KERNEL_CASES:
        case = gc.make_case(name)
        base = {}
        for ks in KEY_SETS:
            keys, topk = ks[:5], ks[5]
            m = reference_match(Ref, case, keys, topk)
            if ks[4]:
                s = case.samples[0]
                ep = O.epipolar_in_box(s.rois, s.npv, s.metas[0]['pad_shape'], O.view_transforms(s.metas), topk, 0.0, 0.0, ks[0], ks[1], ks[2], ks[3])
                want, _ = gc.match_from_lists(case, ep, topk)
                assert np.array_equal(want.numpy(), m), (name, ks, 'oracle.mv2d_oracle.epipolar_in_box differs from the reference')
            if topk not in base:
                base[topk] = reference_match(Ref, case, DEFAULT_KEYS, topk)
            differ = int((m != base[topk]).reshape(case.R, -1).any(1).sum())
            if name == 'r127':
                assert 4 * differ >= case.R, (ks, differ, case.R)
            store['%s_%s' % (name, set_name(ks))] = m
            lines.append('| %s | %s | %d | %d / %d | %d | %d |' % (name, ks, ks[0] * ks[0] * ks[1], differ, case.R, int((m >= 0).sum()),
                                                                   len(TIES[(name, keys, topk)])))
            print(lines[-1], flush=True)
    store['key_sets'] = np.array([[ks[0], ks[1], ks[2], ks[3], float(ks[4]), ks[5]] for ks in KEY_SETS], dtype=np.float64)
    out = os.path.join(OUT, 'box_corr_keys_kernel.npz')
    np.savez_compressed(out, **store)
    assert os.path.getsize(out) < 1024 * 1024, os.path.getsize(out)
    return lines


def build_head(kind, S_cls, T_cls, sd_np, num_views, box_correlation, scale):
    cfg = (configs.roi_head_cfg_s if kind == 'S' else configs.roi_head_cfg_t)(box_correlation=box_correlation, intrins_feat_scale=scale)
    cfg.pop('type')
    cfg['test_cfg'] = configs.TEST_CFG_RCNN
    if kind == 'T':
        cfg['num_views'] = num_views
    head = (S_cls if kind == 'S' else T_cls)(**cfg).eval()
    missing, unexpected = head.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=False)
    assert not unexpected, unexpected
    assert all('loss' in m for m in missing), missing
    bc = dict(dict(ops.BOX_CORR_DEFAULTS), **(box_correlation or {}))
    m = head.box_corr_module
    assert (m.sample_size, m.num_depth, m.depth_start, m.depth_end, m.LID) == tuple(bc[k] for k in ('sample_size', 'num_depth', 'depth_start', 'depth_end', 'LID'))
    assert head.intrins_feat_scale == scale
    return head


def lists_of(rec, kind):
    return (rec['corr'], rec['corr_mask']) if kind == 'S' else (rec['feat_for_rois'],)


def end_to_end(S_cls, T_cls):
    sd_np = synthetic.make_head_state(seed=0)
    store, lines = {}, []
    for name, problem, keys, scale in E2E_CASES:
        for seed in range(MAX_SEED):
            prob = synthetic.make_problem(problem, seed=seed)
            kind = prob['kind']
            torch.set_num_threads(8)
            if keys is not None:
                dflt = run_case(build_head(kind, S_cls, T_cls, sd_np, prob['views_per_frame'], None, 0.1), kind, prob['feat'], prob['proposals'],
                                prob['img_metas'], False)
            recs = {}
            for vname, v in VARIANTS:
                torch.set_num_threads(v['threads'])
                torch.backends.mkldnn.enabled = v['mkldnn']
                head = build_head(kind, S_cls, T_cls, sd_np, prob['views_per_frame'], keys, scale)
                recs[vname] = run_case(head, kind, prob['feat'], prob['proposals'], prob['img_metas'], False)
            torch.backends.mkldnn.enabled = True
            torch.set_num_threads(8)
            base = recs['t8']
            if keys is not None:
                a, b = lists_of(base, kind), lists_of(dflt, kind)
                if all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b)):
                    print(name, 'seed', seed, ': the match lists equal those at the default keys, next seed', flush=True)
                    continue
                assert not np.array_equal(base['intr'], dflt['intr'])
            pair = np.array([[ranked_diff(recs[a]['topk_index'], recs[b]['topk_index']) for b, _ in VARIANTS] for a, _ in VARIANTS], np.int32)
            if int(pair.max()) > NOISE_MAX:
                print(name, 'seed', seed, ': reference rank noise', int(pair.max()), ', next seed', flush=True)
                continue
            break
        else:
            raise AssertionError(name)
        rec = {k: base[k] for k in KEEP if k in base}
        out = os.path.join(OUT, 'box_corr_keys_%s.npz' % name)
        bc = dict(dict(ops.BOX_CORR_DEFAULTS), **(keys or {}))
        np.savez_compressed(out, seed=np.int32(seed), intrins_feat_scale=np.float64(scale), sample_size=np.int32(bc['sample_size']),
                            num_depth=np.int32(bc['num_depth']), depth_start=np.float64(bc['depth_start']), depth_end=np.float64(bc['depth_end']),
                            LID=np.bool_(bc['LID']), **rec)
        assert os.path.getsize(out) < 300 * 1024, (out, os.path.getsize(out))
        gaps = [0.0]
        pos_ = {int(x): j for j, x in enumerate(base['topk_index'])}
        for v, _ in VARIANTS[1:]:
            for i, x in enumerate(recs[v]['topk_index']):
                j = pos_.get(int(x))
                if j is not None and j != i:
                    gaps.append(abs(float(base['topk_scores'][i]) - float(base['topk_scores'][j])))
        store[name + '_variants'] = np.array([v for v, _ in VARIANTS])
        store[name + '_topk_index'] = np.stack([recs[v]['topk_index'] for v, _ in VARIANTS])
        store[name + '_topk_scores'] = np.stack([recs[v]['topk_scores'] for v, _ in VARIANTS])
        store[name + '_pairwise_ranked_diff'] = pair
        store[name + '_max_tie_gap'] = np.float64(max(gaps))
        store[name + '_cls_dev'] = np.float64(max(float(np.abs(recs[v]['cls'] - base['cls']).max()) for v, _ in VARIANTS[1:]) /
                                              float(np.abs(base['cls']).max()))
        if kind == 'S':
            n_keys = '%d matched RoIs' % int(base['corr_mask'].sum())
        else:
            n_keys = '%d key cells' % int(np.unpackbits(base['feat_for_rois']).sum())
        lines.append('| %s | %s | %s | %s | %d | %s | %d | %.1e |' % (name, problem, keys or 'shipped', scale, seed, n_keys, int(pair.max()), max(gaps)))
        print(lines[-1], os.path.getsize(out), 'bytes', flush=True)
    np.savez_compressed(os.path.join(OUT, 'box_corr_keys_refnoise.npz'), **store)
    return lines


README = """# box_corr_keys_*.npz

Written by `tools/gen_golden_box_corr_keys.py` from the unmodified reference; arrays only.  Read by `tests/test_box_corr_keys_cpu.py` and
`tests/test_gpu_box_corr_keys.py`.

## box_corr_keys_kernel.npz

`<layout>_<set>`: `match [R, V, topk]` int32 of the reference's `BoxCorrelation(sample_size, num_depth, depth_start, depth_end, LID,
correlation_mode='topk_matched:<topk>:0.0:0.0').epipolar_in_box` on the RoIs and matrices of `geometry_cases.make_case(<layout>)`, in the
form of `geometry_cases.match_from_lists` (global RoI id at its IoU rank, -1 elsewhere).  `key_sets`: the parameter sets as rows
`(sample_size, num_depth, depth_start, depth_end, LID, topk)`.  For the `LID=True` sets `oracle.mv2d_oracle.epipolar_in_box` gave the same
arrays.  "differ": RoIs whose match row is not the one of the default keys (4, 8, 0.5, 70, LID) at the same topk; on `r127` the generator
asserts at least a quarter.

The reference ranks with an unstable argsort, so RoIs whose IoUs with the epipolar rectangle are equal bit for bit (the layouts hold duplicate
boxes on purpose) come out in either order.  The arrays hold such runs in the order of the RoI index -- the tie rule of the oracle and of the
kernel.  The generator reads the IoUs off the reference's own `box_iou` call and checks every list to be the reference's up to the order inside
such runs.  "tie lists": (RoI, view) lists in which the reference's own order was the other one.

| layout | set | samples | differ | entries >= 0 | tie lists |
|---|---|---|---|---|---|
%s

## box_corr_keys_<case>.npz, box_corr_keys_refnoise.npz

Stage outputs of the reference heads (`oracle.gen_golden.run_case`, the 't8' variant) on `synthetic.make_problem(<problem>, seed)` with
`synthetic.make_head_state(seed=0)`, built from `configs.roi_head_cfg_s / _t(box_correlation=<keys>, intrins_feat_scale=<scale>)`; the keys
and the seed are stored with the arrays.  Seeds are tried from 0; a seed is taken when the match lists (`corr` / `corr_mask`, or
`feat_for_rois`) differ from those of the same head at the default keys and the reference's own ranked decode moves at most %d indices between
its execution variants.  `box_corr_keys_refnoise.npz` holds, per case, the ranked decode of every variant, the pairwise count of moved indices and
the largest score gap across which an index moved.

| case | problem | box_correlation | intrins_feat_scale | seed | keys | ranked indices moved | largest gap |
|---|---|---|---|---|---|---|---|
%s
"""


def main():
    only = [a for a in sys.argv[1:] if not a.startswith('-')]
    S_cls, T_cls = _stubs.install()
    from mmdet3d_plugin.models.roi_heads.utils.box_correlation import BoxCorrelation as Ref      # (importable once _stubs.install has run)
    k_lines = kernel_level(Ref) if not only or 'kernel' in only else None
    e_lines = end_to_end(S_cls, T_cls) if not only or 'e2e' in only else None
    if k_lines is not None and e_lines is not None:
        open(os.path.join(OUT, 'README_box_corr_keys.md'), 'w').write(README % ('\n'.join(k_lines), NOISE_MAX, '\n'.join(e_lines)))


if __name__ == '__main__':
    main()
