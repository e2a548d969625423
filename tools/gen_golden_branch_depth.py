"""Reference goldens for the branch depth ``num_reg_fcs`` (build container only: needs the reference tree; never run on the GPU machine).

    python -B tools/gen_golden_branch_depth.py [case ...]  # writes tests/golden/branch_depth_<case>.npz, branch_depth_refnoise.npz and
                                                           # branch_depth_state_keys.json (described in tests/golden/README_branch_depth.md)

Builds the UNMODIFIED reference MV2DSHead / MV2DTHead with ``bbox_head.num_reg_fcs`` (and, for the RegLayer cases, ``use_reg_layer`` with the case's
``group_reg_dims``) from configs.roi_head_cfg_s / _t(num_reg_fcs=..., reg_layer_dims=...), loads
``synthetic.with_branch_depth_state(make_head_state(seed=0), 0, n, dims)`` and records through ``oracle.gen_golden.run_case`` under every execution
variant of ``oracle.gen_golden_refnoise.VARIANTS``: the 't8' run is the golden (only the keys the tests read are kept, plus ``next_score``, the
best candidate that did not make the top ``max_num``), the others give the reference's own rank noise for that case.

A golden whose ranked scores sit closer together than the engine's class-logit bound can move them decides nothing about ranks, so per case the
problem seed is the first of 0..9 whose golden is DECIDABLE (``decidable`` below, the rule tests/test_branch_depth_cpu.py re-checks); the seed is
recorded in the file (``problem_seed``) and printed for the README table.
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
# (case, problem, num_reg_fcs, group_reg_dims or None = Sequential regression branches): 50-query problems, so the files stay small
CASES = [('n1_cfg1_s', 'cfg1_s', 1, None), ('n3_cfg1_t', 'cfg1_t', 3, None),
         ('n1_rl_cfg1_t', 'cfg1_t', 1, (2, 1, 3, 2, 2)), ('n3_rl_cfg1_s', 'cfg1_s', 3, (2, 2, 1, 1, 2, 2))]
KEEP = ('ref', 'cls', 'reg', 'boxes', 'scores', 'labels', 'topk_index', 'topk_scores')
MAX_NUM, MAX_CLOSE = 300, 8


def tol_cls(n):
    """class-logit bound of the index-exact route against the reference, relative to the largest |logit|: 3e-6 for the shipped chain of two
    split-precision linears, in proportion to their number for a deeper one, no tighter for a shallower one"""
    return 3e-6 * max(n, 2) / 2


def close_entries(scores, eps):
    """entries of the descending score list that have a neighbour closer than eps / 2"""
    s = np.sort(np.asarray(scores, np.float64))[::-1]
    gap = np.abs(np.diff(s)) < eps / 2
    return int((np.concatenate([[False], gap]) | np.concatenate([gap, [False]])).sum())


def decidable(rec, n):
    eps = tol_cls(n) * float(np.abs(rec['cls']).max())
    return close_entries(np.concatenate([rec['topk_scores'], [rec['next_score']]]), eps) <= MAX_CLOSE


def build_head(kind, S_cls, T_cls, sd_np, num_views, n, dims):
    cfg = (configs.roi_head_cfg_s if kind == 'S' else configs.roi_head_cfg_t)(num_reg_fcs=n, reg_layer_dims=dims)
    cfg.pop('type')
    cfg['test_cfg'] = configs.TEST_CFG_RCNN
    if kind == 'T':
        cfg['num_views'] = num_views
    head = (S_cls if kind == 'S' else T_cls)(**cfg).eval()
    missing, unexpected = head.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=False)
    assert not unexpected, unexpected
    assert all('loss' in m for m in missing), missing
    return head


def record(head, prob):
    rec = run_case(head, prob['kind'], prob['feat'], prob['proposals'], prob['img_metas'], False)
    sc = torch.from_numpy(rec['cls'][-1].reshape(-1, 10)).sigmoid().view(-1)
    assert sc.numel() > MAX_NUM, 'the problem has no candidate behind the top max_num'
    top = sc.topk(MAX_NUM + 1)[0].numpy()
    assert np.array_equal(top[:MAX_NUM], rec['topk_scores'])
    rec['next_score'] = np.float32(top[MAX_NUM])
    return rec


def main():
    S_cls, T_cls = _stubs.install(REFERENCE)
    only = [a for a in sys.argv[1:] if not a.startswith('-')]
    path = os.path.join(OUT, 'branch_depth_refnoise.npz')
    store = dict(np.load(path)) if os.path.exists(path) else {}
    kpath = os.path.join(OUT, 'branch_depth_state_keys.json')
    keys = json.load(open(kpath)) if os.path.exists(kpath) else {}
    for name, problem, n, dims in CASES:
        if only and name not in only:
            continue
        sd_np = synthetic.with_branch_depth_state(synthetic.make_head_state(seed=0), 0, n, dims)
        v0 = VARIANTS[0][1]
        for seed in range(10):
            prob = synthetic.make_problem(problem, seed=seed)
            torch.set_num_threads(v0['threads'])
            torch.backends.mkldnn.enabled = v0['mkldnn']
            head = build_head(prob['kind'], S_cls, T_cls, sd_np, prob['views_per_frame'], n, dims)
            first = record(head, prob)
            if decidable(first, n):
                break
            print(f'{name}: problem seed {seed} is not decidable, trying the next', flush=True)
        else:
            raise SystemExit(f'{name}: no decidable problem seed in 0..9')
        recs = {VARIANTS[0][0]: first}
        for vname, v in VARIANTS[1:]:
            torch.set_num_threads(v['threads'])
            torch.backends.mkldnn.enabled = v['mkldnn']
            head = build_head(prob['kind'], S_cls, T_cls, sd_np, prob['views_per_frame'], n, dims)
            recs[vname] = record(head, prob)
        torch.backends.mkldnn.enabled = True
        assert type(head.bbox_head.reg_branches[0]).__name__ == ('RegLayer' if dims else 'Sequential')
        # the reference module's own parameter names and shapes (the plugin head has to build exactly these)
        keys[name] = dict(kind=prob['kind'], problem=problem, problem_seed=seed, num_reg_fcs=n, group_reg_dims=list(dims) if dims else None,
                          bbox_head={k: list(v.shape) for k, v in head.bbox_head.state_dict().items()})
        base = recs['t8']
        np.savez_compressed(os.path.join(OUT, f'branch_depth_{name}.npz'), num_reg_fcs=np.int32(n), problem_seed=np.int32(seed),
                            group_reg_dims=np.array(dims or (), np.int32), next_score=base['next_score'], **{k: base[k] for k in KEEP})
        store[name + '_variants'] = np.array([v for v, _ in VARIANTS])
        store[name + '_topk_index'] = np.stack([recs[v]['topk_index'] for v, _ in VARIANTS])
        store[name + '_topk_scores'] = np.stack([recs[v]['topk_scores'] for v, _ in VARIANTS])
        pair = np.array([[ranked_diff(recs[a]['topk_index'], recs[b]['topk_index']) for b, _ in VARIANTS] for a, _ in VARIANTS], np.int32)
        store[name + '_pairwise_ranked_diff'] = pair
        gaps = [0.0]
        pos = {int(x): j for j, x in enumerate(base['topk_index'])}
        for v, _ in VARIANTS[1:]:
            for i, x in enumerate(recs[v]['topk_index']):
                j = pos.get(int(x))
                if j is not None and j != i:
                    gaps.append(abs(float(base['topk_scores'][i]) - float(base['topk_scores'][j])))
        store[name + '_max_tie_gap'] = np.float64(max(gaps))
        store[name + '_cls_dev'] = np.float64(max(float(np.abs(recs[v]['cls'] - base['cls']).max()) for v, _ in VARIANTS[1:]) /
                                              float(np.abs(base['cls']).max()))
        store[name + '_reg_dev'] = np.float64(max(float(np.abs(recs[v]['reg'] - base['reg']).max()) for v, _ in VARIANTS[1:]))
        np.savez_compressed(path, **store)
        json.dump(keys, open(kpath, 'w'), indent=1, sort_keys=True)
        eps = tol_cls(n) * float(np.abs(base['cls']).max())
        print(name, 'problem seed', seed, {k: base[k].shape for k in KEEP}, 'max ranked diff', int(pair.max()), 'gap %.2e' % max(gaps),
              'eps_n %.2e' % eps, 'close entries', close_entries(np.concatenate([base['topk_scores'], [base['next_score']]]), eps), flush=True)


if __name__ == '__main__':
    main()
