"""Reference goldens for the query generator's shape keys (build container only: needs the reference tree; never run on the GPU machine).

    python -B tools/gen_golden_qg_shape.py [case ...]     # writes tests/golden/qg_shape_<case>.npz, qg_shape_refnoise.npz and
                                                          # qg_shape_state_keys.json (described in tests/golden/README_qg_shape.md)

Builds the UNMODIFIED reference MV2DSHead / MV2DTHead with the case's ``query_generator`` keys (configs.roi_head_cfg_s / _t(query_generator=...,
roi_size=...)), loads ``synthetic.with_qg_shape_state(make_head_state(seed=0), 0, keys, roi_size)`` and records through
``oracle.gen_golden.run_case`` under every execution variant of ``oracle.gen_golden_refnoise.VARIANTS``: the 't8' run is the golden (only the
keys tests/test_gpu_qg_shape.py reads are kept), the others give the reference's own rank noise for that case.  micro_s_c2 additionally records,
through forward hooks on the reference's ``shared_convs[i]``, every conv's output averaged over the cells and the cells of a few RoIs.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mv2d_amd import configs, qg_shape, synthetic  # noqa: E402
from oracle import _stubs  # noqa: E402
from oracle.gen_golden import OUT, run_case  # noqa: E402
from oracle.gen_golden_refnoise import VARIANTS, ranked_diff  # noqa: E402

REFERENCE = '/root/reference'
NOISE_MAX = 4
# (case name, problem, roi_size, query_generator keys)
CASES = [('micro_s_c2', 'micro_s', 7, dict(num_shared_convs=2)),
         ('cfg1_t_c0_f2', 'cfg1_t', 7, dict(num_shared_convs=0, num_shared_fcs=2, fc_out_channels=512, num_center_fcs=1)),
         ('cfg1_s_flat3', 'cfg1_s', 3, dict(with_avg_pool=False)),
         ('cfg1_t_enc', 'cfg1_t', 7, dict(num_shared_convs=3, extra_encoding=dict(num_layers=3, feat_channels=[256, 128, 64], features=[])))]
KEEP = ('intr', 'center_pred', 'xyz', 'feat_for_rois', 'feat_for_rois_shape', 'key_padding', 'corr', 'corr_mask', 'ref', 'cls', 'reg', 'boxes', 'scores',
        'labels', 'topk_index', 'topk_scores')
CELL_ROIS = 2         # micro_s_c2: the conv cells of the first and the last RoI (the file stays under 200 KB)


def case_state(keys, roi_size):
    return synthetic.with_qg_shape_state(synthetic.make_head_state(seed=0), 0, keys, roi_size)


def build_head(kind, S_cls, T_cls, sd_np, num_views, keys, roi_size, train=False):
    cfg = (configs.roi_head_cfg_s if kind == 'S' else configs.roi_head_cfg_t)(query_generator=keys, roi_size=roi_size)
    cfg.pop('type')
    cfg['test_cfg'] = configs.TEST_CFG_RCNN
    if train:
        cfg['train_cfg'] = configs.TRAIN_CFG_RCNN
    if kind == 'T':
        cfg['num_views'] = num_views
    head = (S_cls if kind == 'S' else T_cls)(**cfg).eval()
    missing, unexpected = head.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=False)
    assert not unexpected, unexpected
    assert all('loss' in m for m in missing), missing
    return head


def main():
    S_cls, T_cls = _stubs.install(REFERENCE)
    only = [a for a in sys.argv[1:] if not a.startswith('-')]
    path = os.path.join(OUT, 'qg_shape_refnoise.npz')
    store = dict(np.load(path)) if os.path.exists(path) else {}
    kpath = os.path.join(OUT, 'qg_shape_state_keys.json')
    keys_json = json.load(open(kpath)) if os.path.exists(kpath) else {}
    for name, problem, roi_size, keys in CASES:
        if only and name not in only:
            continue
        sd_np = case_state(keys, roi_size)
        prob = synthetic.make_problem(problem, seed=0)
        recs, convs = {}, {}
        for vname, v in VARIANTS:
            torch.set_num_threads(v['threads'])
            torch.backends.mkldnn.enabled = v['mkldnn']
            head = build_head(prob['kind'], S_cls, T_cls, sd_np, prob['views_per_frame'], keys, roi_size)
            hooks = []
            if name == 'micro_s_c2' and vname == 't8':
                for i, m in enumerate(head.query_generator.shared_convs):
                    hooks.append(m.register_forward_hook(lambda mod, inp, out, i=i: convs.__setitem__(i, out.detach().numpy().copy())))
            recs[vname] = run_case(head, prob['kind'], prob['feat'], prob['proposals'], prob['img_metas'], False)
            for h_ in hooks:
                h_.remove()
        torch.backends.mkldnn.enabled = True
        # the reference module's own parameter names and shapes (the plugin module has to build exactly these)
        qsd = head.query_generator.state_dict()
        shape = qg_shape.parse(keys)
        assert {k: tuple(v.shape) for k, v in qsd.items()} == shape.param_shapes(roi_size)
        keys_json[name] = dict(kind=prob['kind'], problem=problem, roi_size=roi_size, query_generator=keys,
                               params={k: list(v.shape) for k, v in qsd.items()})
        base = recs['t8']
        rec = {k: base[k] for k in KEEP if k in base}
        for i, out in sorted(convs.items()):
            R = out.shape[0]
            rois = np.unique(np.linspace(0, R - 1, CELL_ROIS).astype(np.int64))
            rec[f'conv{i}_pooled'] = out.mean(axis=(2, 3), dtype=np.float64).astype(np.float32)          # [R, 256]
            rec[f'conv{i}_cell_rois'] = rois.astype(np.int32)
            rec[f'conv{i}_cells'] = out[rois].reshape(len(rois), 256, -1).transpose(0, 2, 1).copy()      # [n, s * s, 256], cell-major
        out = os.path.join(OUT, f'qg_shape_{name}.npz')
        np.savez_compressed(out, roi_size=np.int32(roi_size), **rec)
        assert os.path.getsize(out) < 200 * 1024, (out, os.path.getsize(out))
        key = f'{name}_s0'
        store[key + '_variants'] = np.array([v for v, _ in VARIANTS])
        store[key + '_topk_index'] = np.stack([recs[v]['topk_index'] for v, _ in VARIANTS])
        store[key + '_topk_scores'] = np.stack([recs[v]['topk_scores'] for v, _ in VARIANTS])
        pair = np.array([[ranked_diff(recs[a]['topk_index'], recs[b]['topk_index']) for b, _ in VARIANTS] for a, _ in VARIANTS], np.int32)
        store[key + '_pairwise_ranked_diff'] = pair
        assert int(pair.max()) <= NOISE_MAX, (name, int(pair.max()), 'take the next seed and say so in README_qg_shape.md')
        gaps = [0.0]
        pos_ = {int(x): j for j, x in enumerate(base['topk_index'])}
        for v, _ in VARIANTS[1:]:
            for i, x in enumerate(recs[v]['topk_index']):
                j = pos_.get(int(x))
                if j is not None and j != i:
                    gaps.append(abs(float(base['topk_scores'][i]) - float(base['topk_scores'][j])))
        store[key + '_max_tie_gap'] = np.float64(max(gaps))
        store[key + '_cls_dev'] = np.float64(max(float(np.abs(recs[v]['cls'] - base['cls']).max()) for v, _ in VARIANTS[1:]) /
                                             float(np.abs(base['cls']).max()))
        np.savez_compressed(path, **store)
        json.dump(keys_json, open(kpath, 'w'), indent=1, sort_keys=True)
        print(key, {k: v.shape for k, v in rec.items()}, os.path.getsize(out), 'bytes; max ranked diff', int(pair.max()), 'gap %.2e' % max(gaps), flush=True)


if __name__ == '__main__':
    main()
