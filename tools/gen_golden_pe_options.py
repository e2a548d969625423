"""Reference goldens for the PE's with_fpe / no_sin_enc / adapt_pos3d / LID keys (build container only: needs the reference tree; never run on the GPU machine).

    python -B tools/gen_golden_pe_options.py [case ...]   # writes tests/golden/pe_options_<case>.npz, pe_options_refnoise.npz and
                                                          # pe_options_state_keys.json (described in tests/golden/README_pe_options.md)

Builds the UNMODIFIED reference MV2DSHead / MV2DTHead with the case's ``pe`` keys (configs.roi_head_cfg_s / _t(with_fpe=..., no_sin_enc=...,
adapt_pos3d=..., LID=..., depth_num=...)), loads ``synthetic.with_pe_options_state`` of the seed-0 head state (after ``with_pe_depth_state`` for
another depth_num) with no unexpected and no missing key, and records through ``oracle.gen_golden.run_case`` under every execution variant of
``oracle.gen_golden_refnoise.VARIANTS``: the 't8' run is the golden (only the keys tests/test_gpu_pe_options.py reads are kept), the others give the
reference's own rank noise for that case.  Rank noise is a CONDITION: a case whose variants disagree in more than NOISE_MAX ranked indices takes the
next problem seed (the seed used is stored in the file and named in the README).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mv2d_amd import configs, ops, synthetic  # noqa: E402
from oracle import _stubs  # noqa: E402
from oracle.gen_golden import OUT, run_case  # noqa: E402
from oracle.gen_golden_refnoise import VARIANTS, ranked_diff  # noqa: E402

REFERENCE = '/root/reference'
NOISE_MAX = 4
MAX_SEED = 4
# (case name, problem, pe keys): the gate-less kernel pe-only (S path) with pe rows; the gate-less kernel with key / value rows (T path); the shipped
# gated kernel on a zero table with uniform bins; everything off at once at 40 bins (Kp = 128 with 8 pad columns) with pe rows
CASES = [('micro_s_nofpe', 'micro_s', dict(with_fpe=False)),
         ('cfg1_t_nofpe', 'cfg1_t', dict(with_fpe=False)),
         ('cfg1_s_nosin_uni', 'cfg1_s', dict(no_sin_enc=True, LID=False)),
         ('micro_t_plain_d40', 'micro_t', dict(with_fpe=False, no_sin_enc=True, adapt_pos3d=False, LID=False, depth_num=40))]
KEEP = ('intr', 'center_pred', 'xyz', 'feat_for_rois', 'feat_for_rois_shape', 'key_padding', 'corr', 'corr_mask', 'ref', 'cls', 'reg', 'boxes', 'scores',
        'labels', 'topk_index', 'topk_scores')
PE_STEP = 3           # the micro cases: the reference's pe map at every third map position (the files stay under 200 KB)


def case_state(pe_keys):
    """The seed-0 head state laid out for the case's PE: another depth_num's first layer, then without the submodules the switches leave out."""
    sd = synthetic.make_head_state(seed=0)
    D = pe_keys.get('depth_num', 64)
    if D != 64:
        sd = synthetic.with_pe_depth_state(sd, 0, D)
    return synthetic.with_pe_options_state(sd, pe_keys.get('with_fpe', True), pe_keys.get('no_sin_enc', False))


def build_head(kind, S_cls, T_cls, sd_np, num_views, pe_keys, train_cfg=None):
    cfg = configs.roi_head_cfg_s(**pe_keys) if kind == 'S' else configs.roi_head_cfg_t(**pe_keys)
    cfg.pop('type')
    cfg['test_cfg'] = configs.TEST_CFG_RCNN
    if train_cfg is not None:
        cfg['train_cfg'] = train_cfg
    if kind == 'T':
        cfg['num_views'] = num_views
    head = (S_cls if kind == 'S' else T_cls)(**cfg).eval()
    missing, unexpected = head.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=False)
    assert not unexpected, unexpected
    assert all('loss' in m for m in missing), missing
    pe = head.position_encoding
    o = {**ops.PE_OPTION_DEFAULTS, **{k: v for k, v in pe_keys.items() if k in ops.PE_OPTION_DEFAULTS}}
    assert pe.with_fpe == o['with_fpe'] and pe.no_sin_enc == o['no_sin_enc'] and pe.LID == o['LID'] and pe.depth_num == pe_keys.get('depth_num', 64)
    assert hasattr(pe, 'fpe') == o['with_fpe'] and hasattr(pe, 'adapt_pos3d') == (not o['no_sin_enc']) == hasattr(pe, 'positional_encoding')
    return head


def record(S_cls, T_cls, name, problem, pe_keys, seed):
    sd_np = case_state(pe_keys)
    prob = synthetic.make_problem(problem, seed=seed)
    full = problem.startswith('micro')
    recs = {}
    for vname, v in VARIANTS:
        torch.set_num_threads(v['threads'])
        torch.backends.mkldnn.enabled = v['mkldnn']
        head = build_head(prob['kind'], S_cls, T_cls, sd_np, prob['views_per_frame'], pe_keys)
        recs[vname] = run_case(head, prob['kind'], prob['feat'], prob['proposals'], prob['img_metas'], full and vname == 't8')
    torch.backends.mkldnn.enabled = True
    pair = np.array([[ranked_diff(recs[a]['topk_index'], recs[b]['topk_index']) for b, _ in VARIANTS] for a, _ in VARIANTS], np.int32)
    return prob, head, recs, pair, full


def main():
    S_cls, T_cls = _stubs.install(REFERENCE)
    only = [a for a in sys.argv[1:] if not a.startswith('-')]
    path = os.path.join(OUT, 'pe_options_refnoise.npz')
    store = dict(np.load(path)) if os.path.exists(path) else {}
    kpath = os.path.join(OUT, 'pe_options_state_keys.json')
    keys = json.load(open(kpath)) if os.path.exists(kpath) else {}
    for name, problem, pe_keys in CASES:
        if only and name not in only:
            continue
        for seed in range(MAX_SEED + 1):
            prob, head, recs, pair, full = record(S_cls, T_cls, name, problem, pe_keys, seed)
            if int(pair.max()) <= NOISE_MAX:
                break
            print(name, 'seed', seed, ': the reference variants differ in', int(pair.max()), 'ranked indices -> next seed', flush=True)
        assert int(pair.max()) <= NOISE_MAX, (name, int(pair.max()))
        o = {**ops.PE_OPTION_DEFAULTS, **{k: v for k, v in pe_keys.items() if k in ops.PE_OPTION_DEFAULTS}}
        D = pe_keys.get('depth_num', 64)
        # the reference module's own parameter names and shapes (the plugin PE has to build exactly these)
        keys[name] = dict(kind=prob['kind'], problem=problem, seed=seed, depth_num=D, **o,
                          position_encoding={k: list(v.shape) for k, v in head.position_encoding.state_dict().items()})
        base = recs['t8']
        rec = {k: base[k] for k in KEEP if k in base}
        if full:
            V, C, h, w = base['pe'].shape
            pos = np.arange(0, V * h * w, PE_STEP, dtype=np.int32)
            rec['pe_positions'] = pos                                                     # flat (view, y, x) map positions
            rec['pe_rows'] = base['pe'].transpose(0, 2, 3, 1).reshape(V * h * w, C)[pos]   # [len(pos), 256]
        out = os.path.join(OUT, f'pe_options_{name}.npz')
        np.savez_compressed(out, seed=np.int32(seed), depth_num=np.int32(D), **{k: np.bool_(v) for k, v in o.items()}, **rec)
        assert os.path.getsize(out) < 200 * 1024, (out, os.path.getsize(out))
        key = f'{name}_s{seed}'
        for k in [k for k in store if k.startswith(name + '_s')]:
            del store[k]
        store[key + '_variants'] = np.array([v for v, _ in VARIANTS])
        store[key + '_topk_index'] = np.stack([recs[v]['topk_index'] for v, _ in VARIANTS])
        store[key + '_topk_scores'] = np.stack([recs[v]['topk_scores'] for v, _ in VARIANTS])
        store[key + '_pairwise_ranked_diff'] = pair
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
