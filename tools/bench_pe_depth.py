#!/usr/bin/env python
"""What the number of PE depth bins costs (GPU only): samples/s of one engine at depth_num 32, 64 and 80.

    python tools/bench_pe_depth.py [--samples 16] [--calls 20] [--runs 3] [--depths 32 64 80] [--workloads cfg3_t cfg2_s]
                                   [--parent-root DIR]

Every (workload, depth) is measured in a child process of its own (one engine on one stream, run_batch of --samples samples, graph replay,
--calls calls per run), the median of --runs runs is reported; the children run one after the other, the depths alternating inside a run.
Not bench.py's number: that runs four streams with rotating inputs.

--parent-root DIR: a BUILT checkout of another commit (its own mv2d_amd package and library).  depth_num = 64 is then timed in that checkout
and in this one, alternating, --runs times each: the 64-bin kernels are the same instruction streams, so the two must agree within the
run-to-run spread, which is printed next to the difference.

The kernel time of the fused PE launch at each depth comes from a separate profiler run of the child mode:

    rocprofv3 --kernel-trace --stats -- python tools/bench_pe_depth.py --one cfg3_t 32
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(root, workload, depth, samples, calls):
    """Child mode: one JSON line with samples/s.  `root`: the checkout whose package is imported (depth 64 only needs what every commit has)."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from mv2d_amd import synthetic
    from mv2d_amd.engine import HeadEngine
    dev = torch.device('cuda:0')
    sd = synthetic.make_head_state(seed=0)
    if depth != 64:
        sd = synthetic.with_pe_depth_state(sd, 0, depth)
    probs = [synthetic.make_problem(workload, seed=s) for s in range(samples)]
    eng = HeadEngine(sd, probs[0]['kind'], dev, num_views=probs[0]['views_per_frame'], depth_num=depth)
    feats = torch.cat([torch.from_numpy(p['feat']) for p in probs]).to(dev)
    props = [[torch.from_numpy(np.asarray(x)) for x in p['proposals']] for p in probs]
    metas = [p['img_metas'] for p in probs]
    for _ in range(5):
        eng.run_batch(feats, props, metas, use_graph=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        eng.run_batch(feats, props, metas, use_graph=True)
    torch.cuda.synchronize()
    print(json.dumps(dict(workload=workload, depth_num=depth, samples_s=calls * samples / (time.perf_counter() - t0), root=root)), flush=True)


def child(root, workload, depth, args):
    cmd = [sys.executable, os.path.abspath(__file__), '--one', workload, str(depth), '--root', root, '--samples', str(args.samples), '--calls', str(args.calls)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
    if r.returncode != 0:
        # a child that faulted, aborted or hung ends the measurement: nothing more is started on the device
        sys.exit(f'child {cmd} ended with status {r.returncode}:\n{r.stderr[-2000:]}')
    return json.loads(r.stdout.strip().splitlines()[-1])['samples_s']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--one', nargs=2, metavar=('WORKLOAD', 'DEPTH'))
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--depths', type=int, nargs='+', default=[32, 64, 80])
    ap.add_argument('--workloads', nargs='+', default=['cfg3_t', 'cfg2_s'])
    ap.add_argument('--parent-root', default=None)
    ap.add_argument('--child-timeout', type=int, default=240)
    args = ap.parse_args()
    if args.one:
        return one(args.root, args.one[0], int(args.one[1]), args.samples, args.calls)
    print(f'# samples/s, one engine on one stream, run_batch of {args.samples} samples, graph replay, {args.calls} calls per run, median of {args.runs} runs '
          f'(one child process per run, depths alternating)')
    for wl in args.workloads:
        rates = {d: [] for d in args.depths}
        for _ in range(args.runs):
            for d in args.depths:
                rates[d].append(child(HERE, wl, d, args))
        for d, v in rates.items():
            print(f'{wl:8s} depth_num {d:3d}: median {statistics.median(v):8.1f}   min {min(v):8.1f}   max {max(v):8.1f} samples/s', flush=True)
        if args.parent_root:
            both = {'this checkout': [], 'parent checkout': []}
            for _ in range(args.runs):
                both['this checkout'].append(child(HERE, wl, 64, args))
                both['parent checkout'].append(child(os.path.abspath(args.parent_root), wl, 64, args))
            med = {k: statistics.median(v) for k, v in both.items()}
            spread = max((max(v) - min(v)) / statistics.median(v) for v in both.values())
            for k, v in both.items():
                print(f'{wl:8s} depth_num  64, {k:15s}: median {med[k]:8.1f}   min {min(v):8.1f}   max {max(v):8.1f} samples/s', flush=True)
            print(f'{wl:8s} depth_num  64: this / parent = {med["this checkout"] / med["parent checkout"]:.4f}, run-to-run spread (max - min) / median = {spread:.4f}', flush=True)


if __name__ == '__main__':
    main()
