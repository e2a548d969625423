"""Reference goldens for class counts other than 10 (build container only: needs the reference tree; never run on the GPU machine).

    python -B tools/gen_golden_num_classes.py [case ...]     # writes tests/golden/ncls_<case>_n<N>.npz + tests/golden/ncls_refnoise.npz
                                                            # (described in tests/golden/README_ncls.md)

Builds the UNMODIFIED reference MV2DSHead / MV2DTHead with ``num_classes = N`` in both ``bbox_head`` and ``bbox_head.bbox_coder``
(configs.roi_head_cfg_s / _t(num_classes=N)), loads ``synthetic.make_head_state(seed=0, num_classes=N)`` and records through
``oracle.gen_golden.run_case`` under every execution variant of ``oracle.gen_golden_refnoise.VARIANTS``: the 't8' run is the golden, the
others give the reference's own rank noise for that case (same keys as refnoise.npz, in a file of its own).  ``run_case`` ranks with a
fixed 10 columns, so the flat top-300 indices are recomputed here from the recorded class logits.
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
CASES = [('cfg2_s', 3), ('cfg3_t', 1), ('cfg5_t', 26)]        # S headline size; T single class; 900 queries x 26 = 23 400 candidates


def build_head(kind, S_cls, T_cls, sd_np, num_views, N):
    cfg = configs.roi_head_cfg_s(num_classes=N) if kind == 'S' else configs.roi_head_cfg_t(num_classes=N)
    cfg.pop('type')
    cfg['test_cfg'] = configs.TEST_CFG_RCNN
    if kind == 'T':
        cfg['num_views'] = num_views
    head = (S_cls if kind == 'S' else T_cls)(**cfg).eval()
    missing, unexpected = head.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=False)
    assert not unexpected, unexpected
    assert all('loss' in m for m in missing), missing
    return head


def rerank(rec, N):
    """the flat (query, class) top-k of the last layer's logits, as CB/coders/nms_free_coder.py:66 does it"""
    cls_last = torch.from_numpy(rec['cls'][-1].reshape(-1, N))
    sc, idx = cls_last.sigmoid().view(-1).topk(min(300, cls_last.numel()))
    rec.update(topk_index=idx.numpy(), topk_scores=sc.numpy())
    return rec


def main():
    S_cls, T_cls = _stubs.install(REFERENCE)
    only = [a for a in sys.argv[1:] if not a.startswith('-')]
    path = os.path.join(OUT, 'ncls_refnoise.npz')
    store = dict(np.load(path)) if os.path.exists(path) else {}
    for name, N in CASES:
        if only and name not in only:
            continue
        sd_np = synthetic.make_head_state(seed=0, num_classes=N)
        prob = synthetic.make_problem(name, seed=0)
        recs = {}
        for vname, v in VARIANTS:
            torch.set_num_threads(v['threads'])
            torch.backends.mkldnn.enabled = v['mkldnn']
            head = build_head(prob['kind'], S_cls, T_cls, sd_np, prob['views_per_frame'], N)
            recs[vname] = rerank(run_case(head, prob['kind'], prob['feat'], prob['proposals'], prob['img_metas'], False), N)
        torch.backends.mkldnn.enabled = True
        base = recs['t8']
        assert base['cls'].shape[-1] == N and int(base['labels'].max(initial=0)) < N
        np.savez_compressed(os.path.join(OUT, f'ncls_{name}_n{N}.npz'), **base)
        key = f'{name}_n{N}_s0'
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
