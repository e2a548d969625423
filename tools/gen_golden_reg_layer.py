"""Reference goldens for the RegLayer regression branches (build container only: needs the reference tree; never run on the GPU machine).

    python -B tools/gen_golden_reg_layer.py [case ...]    # writes tests/golden/reg_layer_<case>.npz, reg_layer_refnoise.npz and
                                                          # reg_layer_state_keys.json (described in tests/golden/README_reg_layer.md)

Builds the UNMODIFIED reference MV2DSHead / MV2DTHead with ``bbox_head.use_reg_layer=True`` and the case's ``group_reg_dims``
(configs.roi_head_cfg_s / _t(reg_layer_dims=...)), loads ``synthetic.with_reg_layer_state(make_head_state(seed=0), 0, dims)`` and records
through ``oracle.gen_golden.run_case`` under every execution variant of ``oracle.gen_golden_refnoise.VARIANTS``: the 't8' run is the golden
(only the keys tests/test_gpu_reg_layer.py reads are kept), the others give the reference's own rank noise for that case.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mv2d_amd import configs, synthetic  # noqa: E402
from oracle import _stubs  # noqa: E402
from oracle.gen_golden import OUT, run_case  # noqa: E402
from oracle.gen_golden_refnoise import VARIANTS, ranked_diff  # noqa: E402

REFERENCE = '/root/reference'
# (case name, problem, group_reg_dims): the head's default; RegLayer's own default; two frames, so that dt divides the velocity
CASES = [('cfg1_s', 'cfg1_s', (2, 2, 1, 1, 2, 2)), ('cfg1_t', 'cfg1_t', (2, 1, 3, 2, 2)), ('cfg3_t', 'cfg3_t', (2, 2, 1, 1, 2, 2))]
KEEP = ('ref', 'cls', 'reg', 'boxes', 'scores', 'labels', 'topk_index', 'topk_scores')


def build_head(kind, S_cls, T_cls, sd_np, num_views, dims):
    cfg = configs.roi_head_cfg_s(reg_layer_dims=dims) if kind == 'S' else configs.roi_head_cfg_t(reg_layer_dims=dims)
    cfg.pop('type')
    cfg['test_cfg'] = configs.TEST_CFG_RCNN
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
    path = os.path.join(OUT, 'reg_layer_refnoise.npz')
    store = dict(np.load(path)) if os.path.exists(path) else {}
    kpath = os.path.join(OUT, 'reg_layer_state_keys.json')
    keys = json.load(open(kpath)) if os.path.exists(kpath) else {}
    for name, problem, dims in CASES:
        if only and name not in only:
            continue
        sd_np = synthetic.with_reg_layer_state(synthetic.make_head_state(seed=0), 0, dims)
        prob = synthetic.make_problem(problem, seed=0)
        recs = {}
        for vname, v in VARIANTS:
            torch.set_num_threads(v['threads'])
            torch.backends.mkldnn.enabled = v['mkldnn']
            head = build_head(prob['kind'], S_cls, T_cls, sd_np, prob['views_per_frame'], dims)
            assert type(head.bbox_head.reg_branches[0]).__name__ == 'RegLayer'
            recs[vname] = run_case(head, prob['kind'], prob['feat'], prob['proposals'], prob['img_metas'], False)
        torch.backends.mkldnn.enabled = True
        # the reference module's own parameter names and shapes (the plugin head has to build exactly these)
        keys[name] = dict(kind=prob['kind'], group_reg_dims=list(dims),
                          bbox_head={k: list(v.shape) for k, v in head.bbox_head.state_dict().items()})
        base = recs['t8']
        np.savez_compressed(os.path.join(OUT, f'reg_layer_{name}.npz'), group_reg_dims=np.array(dims, np.int32), **{k: base[k] for k in KEEP})
        key = f'{name}_s0'
        store[key + '_variants'] = np.array([v for v, _ in VARIANTS])
        store[key + '_topk_index'] = np.stack([recs[v]['topk_index'] for v, _ in VARIANTS])
        store[key + '_topk_scores'] = np.stack([recs[v]['topk_scores'] for v, _ in VARIANTS])
        pair = np.array([[ranked_diff(recs[a]['topk_index'], recs[b]['topk_index']) for b, _ in VARIANTS] for a, _ in VARIANTS], np.int32)
        store[key + '_pairwise_ranked_diff'] = pair
        gaps = [0.0]
        pos = {int(x): j for j, x in enumerate(base['topk_index'])}
        for v, _ in VARIANTS[1:]:
            for i, x in enumerate(recs[v]['topk_index']):
                j = pos.get(int(x))
                if j is not None and j != i:
                    gaps.append(abs(float(base['topk_scores'][i]) - float(base['topk_scores'][j])))
        store[key + '_max_tie_gap'] = np.float64(max(gaps))
        store[key + '_cls_dev'] = np.float64(max(float(np.abs(recs[v]['cls'] - base['cls']).max()) for v, _ in VARIANTS[1:]) /
                                             float(np.abs(base['cls']).max()))
        store[key + '_reg_dev'] = np.float64(max(float(np.abs(recs[v]['reg'] - base['reg']).max()) for v, _ in VARIANTS[1:]))
        np.savez_compressed(path, **store)
        json.dump(keys, open(kpath, 'w'), indent=1, sort_keys=True)
        print(key, {k: base[k].shape for k in KEEP}, 'max ranked diff', int(pair.max()), 'gap %.2e' % max(gaps), flush=True)


if __name__ == '__main__':
    main()
