#!/usr/bin/env python
"""Run the engine at one query-generator shape case (GPU only), for a profiler run of its own:

    rocprofv3 --kernel-trace --stats -- python tools/run_qg_shape.py micro_s_c2 [--calls 20]

The cases are those of tools/gen_golden_qg_shape.py (tests/golden/qg_shape_state_keys.json) plus `default` (the shipped shape on cfg1_s).  Eager
runs of one sample on one stream; the kernels of the new launches are roi_conv_cells_kernel<true> and avgpool_cells_kernel (csrc/roiconv_cells.hip)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('case')
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    from mv2d_amd import synthetic
    from mv2d_amd.engine import HeadEngine
    keys = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'qg_shape_state_keys.json')))
    rec = dict(problem='cfg1_s', roi_size=7, query_generator=None) if args.case == 'default' else keys[args.case]
    prob = synthetic.make_problem(rec['problem'], seed=0)
    sd = synthetic.make_head_state(seed=0)
    if rec['query_generator']:
        sd = synthetic.with_qg_shape_state(sd, 0, rec['query_generator'], rec['roi_size'])
    dev = torch.device('cuda:0')
    eng = HeadEngine(sd, prob['kind'], dev, num_views=prob['views_per_frame'], roi_size=rec['roi_size'], query_generator=rec['query_generator'])
    feat = torch.from_numpy(prob['feat']).to(dev)
    props = [torch.from_numpy(np.asarray(p)) for p in prob['proposals']]
    for _ in range(args.calls):
        out = eng.run(feat, props, prob['img_metas'])
    torch.cuda.synchronize()
    print(json.dumps(dict(case=args.case, R=out['R'], boxes=int(out['count'][0]), calls=args.calls)))


if __name__ == '__main__':
    main()
