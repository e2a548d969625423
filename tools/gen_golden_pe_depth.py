"""Reference goldens for the PE's depth_num / depth_start / position_range (build container only: needs the reference tree; never run on the GPU machine).

    python -B tools/gen_golden_pe_depth.py [case ...]     # writes tests/golden/pe_depth_<case>.npz, pe_depth_refnoise.npz and
                                                          # pe_depth_state_keys.json (described in tests/golden/README_pe_depth.md)

Builds the UNMODIFIED reference MV2DSHead / MV2DTHead with the case's ``pe`` keys (configs.roi_head_cfg_s / _t(depth_num=..., depth_start=...,
position_range=...)), loads ``synthetic.with_pe_depth_state(make_head_state(seed=0), 0, depth_num)`` and records through
``oracle.gen_golden.run_case`` under every execution variant of ``oracle.gen_golden_refnoise.VARIANTS``: the 't8' run is the golden (only the
keys tests/test_gpu_pe_depth.py reads are kept), the others give the reference's own rank noise for that case.
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
NOISE_MAX = 4
# (case name, problem, pe keys): one first-layer k-step; no padding, three k-steps; 8 pad columns with both other keys off what the coder's range
# and the default start would give; eight k-steps on two frames (velocity / dt tail)
CASES = [('micro_s_d8', 'micro_s', dict(depth_num=8)),
         ('cfg1_s_d32', 'cfg1_s', dict(depth_num=32)),
         ('cfg1_t_d40', 'cfg1_t', dict(depth_num=40, depth_start=2.0, position_range=[-65.0, -65.0, -8.0, 65.0, 65.0, 8.0])),
         ('cfg3_t_d80', 'cfg3_t', dict(depth_num=80))]
KEEP = ('intr', 'center_pred', 'xyz', 'feat_for_rois', 'feat_for_rois_shape', 'key_padding', 'corr', 'corr_mask', 'ref', 'cls', 'reg', 'boxes', 'scores',
        'labels', 'topk_index', 'topk_scores')
PE_STEP = 3           # micro_s_d8: the reference's pe map at every third position of the 2 x 8 x 12 map (64 rows: the file stays under 200 KB)


def build_head(kind, S_cls, T_cls, sd_np, num_views, pe_keys):
    cfg = configs.roi_head_cfg_s(**pe_keys) if kind == 'S' else configs.roi_head_cfg_t(**pe_keys)
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
    path = os.path.join(OUT, 'pe_depth_refnoise.npz')
    store = dict(np.load(path)) if os.path.exists(path) else {}
    kpath = os.path.join(OUT, 'pe_depth_state_keys.json')
    keys = json.load(open(kpath)) if os.path.exists(kpath) else {}
    for name, problem, pe_keys in CASES:
        if only and name not in only:
            continue
        D = pe_keys['depth_num']
        sd_np = synthetic.with_pe_depth_state(synthetic.make_head_state(seed=0), 0, D)
        prob = synthetic.make_problem(problem, seed=0)
        full = name == 'micro_s_d8'
        recs = {}
        for vname, v in VARIANTS:
            torch.set_num_threads(v['threads'])
            torch.backends.mkldnn.enabled = v['mkldnn']
            head = build_head(prob['kind'], S_cls, T_cls, sd_np, prob['views_per_frame'], pe_keys)
            pe = head.position_encoding
            assert pe.depth_num == D and tuple(pe.position_encoder[0].weight.shape) == (1024, 3 * D, 1, 1)
            assert float(pe.depth_start) == float(pe_keys.get('depth_start', 1)) and list(pe.position_range) == list(pe_keys.get('position_range', configs.POST_RANGE))
            recs[vname] = run_case(head, prob['kind'], prob['feat'], prob['proposals'], prob['img_metas'], full and vname == 't8')
        torch.backends.mkldnn.enabled = True
        # the reference module's own parameter names and shapes (the plugin PE has to build exactly these)
        keys[name] = dict(kind=prob['kind'], depth_num=D, position_encoding={k: list(v.shape) for k, v in head.position_encoding.state_dict().items()})
        base = recs['t8']
        rec = {k: base[k] for k in KEEP if k in base}
        if full:
            V, C, h, w = base['pe'].shape
            pos = np.arange(0, V * h * w, PE_STEP, dtype=np.int32)
            rec['pe_positions'] = pos                                                     # flat (view, y, x) map positions
            rec['pe_rows'] = base['pe'].transpose(0, 2, 3, 1).reshape(V * h * w, C)[pos]   # [len(pos), 256]
        out = os.path.join(OUT, f'pe_depth_{name}.npz')
        np.savez_compressed(out, depth_num=np.int32(D), depth_start=np.float64(pe_keys.get('depth_start', 1)),
                            position_range=np.array(pe_keys.get('position_range', configs.POST_RANGE), np.float64), **rec)
        assert os.path.getsize(out) < 200 * 1024, (out, os.path.getsize(out))
        key = f'{name}_s0'
        store[key + '_variants'] = np.array([v for v, _ in VARIANTS])
        store[key + '_topk_index'] = np.stack([recs[v]['topk_index'] for v, _ in VARIANTS])
        store[key + '_topk_scores'] = np.stack([recs[v]['topk_scores'] for v, _ in VARIANTS])
        pair = np.array([[ranked_diff(recs[a]['topk_index'], recs[b]['topk_index']) for b, _ in VARIANTS] for a, _ in VARIANTS], np.int32)
        store[key + '_pairwise_ranked_diff'] = pair
        assert int(pair.max()) <= NOISE_MAX, (name, int(pair.max()), 'take the next seed and say so in README_pe_depth.md')
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
        json.dump(keys, open(kpath, 'w'), indent=1, sort_keys=True)
        print(key, {k: v.shape for k, v in rec.items()}, os.path.getsize(out), 'bytes; max ranked diff', int(pair.max()), 'gap %.2e' % max(gaps), flush=True)


if __name__ == '__main__':
    main()
