"""Reference goldens for RoI sizes other than 7 (build container only: needs the reference tree; never run on the GPU machine).

    python -B tools/gen_golden_roi_size.py [case ...]     # writes tests/golden/roi_size_<case>_s<s>.npz + tests/golden/roi_size_refnoise.npz
                                                         # (described in tests/golden/README_roi_size.md)

Builds the UNMODIFIED reference MV2DSHead / MV2DTHead with ``roi_size = s`` in the RoI extractor's RoIAlign and in the query generator
(configs.roi_head_cfg_s / _t(roi_size=s); the stub SingleRoIExtractor passes ``output_size`` on), loads ``synthetic.make_head_state(seed=0)``
(no weight shape depends on s) and records through ``oracle.gen_golden.run_case`` under every execution variant of
``oracle.gen_golden_refnoise.VARIANTS``: the 't8' run is the golden, the others give the reference's own rank noise for that case (same keys
as refnoise.npz, in a file of its own).  The training case (``train`` on the command line) is written by tools/gen_golden_roi_size_train.py.
"""
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
CASES = [('cfg2_s', 5), ('cfg3_t', 9), ('nc6_s', 14), ('cfg1_s', 1)]   # S headline size; T above 7; up to 6 x 196 keys per query; one key per RoI


def build_head(kind, S_cls, T_cls, sd_np, num_views, s):
    cfg = configs.roi_head_cfg_s(roi_size=s) if kind == 'S' else configs.roi_head_cfg_t(roi_size=s)
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
    path = os.path.join(OUT, 'roi_size_refnoise.npz')
    store = dict(np.load(path)) if os.path.exists(path) else {}
    for name, rs in CASES:
        if only and name not in only:
            continue
        sd_np = synthetic.make_head_state(seed=0)
        prob = synthetic.make_problem(name, seed=0)
        recs = {}
        for vname, v in VARIANTS:
            torch.set_num_threads(v['threads'])
            torch.backends.mkldnn.enabled = v['mkldnn']
            head = build_head(prob['kind'], S_cls, T_cls, sd_np, prob['views_per_frame'], rs)
            assert head.bbox_roi_extractor.cfg[0] == rs          # the stub extractor's RoIAlign output size
            recs[vname] = run_case(head, prob['kind'], prob['feat'], prob['proposals'], prob['img_metas'], False)
        torch.backends.mkldnn.enabled = True
        base = recs['t8']
        np.savez_compressed(os.path.join(OUT, f'roi_size_{name}_s{rs}.npz'), **base)
        key = f'{name}_s{rs}_s0'
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
        np.savez_compressed(path, **store)
        print(key, {k: v.shape for k, v in base.items()}, 'max ranked diff', int(pair.max()), 'gap %.2e' % max(gaps), flush=True)


if __name__ == '__main__':
    main()
