#!/usr/bin/env python
"""What the branch depth (HeadEngine(num_reg_fcs=n)) costs next to the shipped depth (GPU only).

    python tools/bench_branch_depth.py [--samples 16] [--rounds 3]

Samples/s of ONE engine on ONE stream: run_batch of --samples samples per call, graph replay, for cfg2_s and cfg3_t at n = 1, 2, 3 (2 = the
shipped kernels, the same run's yardstick), the depths ALTERNATING inside one process; the median of --rounds rounds of 20 calls.  Not bench.py's
number: that runs four streams with rotating inputs."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mv2d_amd import synthetic  # noqa: E402
from mv2d_amd.engine import HeadEngine  # noqa: E402

DEV = torch.device('cuda:0')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    B = args.samples
    base = synthetic.make_head_state(seed=0)
    for name in ('cfg2_s', 'cfg3_t'):
        probs = [synthetic.make_problem(name, seed=s) for s in range(B)]
        feats = torch.cat([torch.from_numpy(p['feat']) for p in probs]).to(DEV)
        props = [[torch.from_numpy(np.asarray(x)) for x in p['proposals']] for p in probs]
        metas = [p['img_metas'] for p in probs]
        kind, views = probs[0]['kind'], probs[0]['views_per_frame']
        engs = {n: HeadEngine(base if n == 2 else synthetic.with_branch_depth_state(base, 0, n), kind, DEV, num_views=views, num_reg_fcs=n)
                for n in (1, 2, 3)}
        for e in engs.values():
            for _ in range(3):
                e.run_batch(feats, props, metas, use_graph=True)
        torch.cuda.synchronize()
        rates = {n: [] for n in engs}
        for _ in range(args.rounds):
            for n, e in engs.items():
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    e.run_batch(feats, props, metas, use_graph=True)
                torch.cuda.synchronize()
                rates[n].append(args.calls * B / (time.perf_counter() - t0))
        print(f'# {name}: samples/s, one engine on one stream, run_batch of {B} samples, graph replay, median of {args.rounds} alternating rounds '
              f'of {args.calls} calls')
        for n, v in rates.items():
            print(f'{name} num_reg_fcs={n}{" (shipped kernels)" if n == 2 else "":18s} median {statistics.median(v):8.1f}   max {max(v):8.1f} samples/s', flush=True)


if __name__ == '__main__':
    main()
