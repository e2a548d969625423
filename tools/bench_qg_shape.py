#!/usr/bin/env python
"""Does the default query-generator shape cost what it cost at the parent commit (GPU only)?

    python tools/bench_qg_shape.py --parent-root DIR [--samples 16] [--calls 20] [--runs 5] [--workloads cfg2_s cfg3_t]

The protocol of tools/bench_pe_depth.py (its child mode is what runs: one engine on one stream, run_batch of --samples samples, graph replay, --calls
calls per run, one child process per run): the default shape in this checkout and in DIR, a BUILT checkout of the parent commit, alternating, --runs
times each.  Printed per workload: both medians, their ratio, and the spread the parent shows against itself in the same call, (max - min) / median of
its own runs -- the allowed difference."""
import argparse
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, 'tools'))
import bench_pe_depth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-root', required=True)
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--workloads', nargs='+', default=['cfg2_s', 'cfg3_t'])
    ap.add_argument('--child-timeout', type=int, default=240)
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_root)
    print(f'# samples/s at the default query-generator shape, one engine on one stream, run_batch of {args.samples} samples, graph replay, {args.calls} calls per '
          f'run, {args.runs} runs each (one child process per run, the two checkouts alternating)')
    for wl in args.workloads:
        rates = {'this checkout': [], 'parent checkout': []}
        for _ in range(args.runs):
            rates['this checkout'].append(bench_pe_depth.child(HERE, wl, 64, args))
            rates['parent checkout'].append(bench_pe_depth.child(parent, wl, 64, args))
        med = {k: statistics.median(v) for k, v in rates.items()}
        for k, v in rates.items():
            print(f'{wl:8s} {k:15s}: median {med[k]:8.1f}   min {min(v):8.1f}   max {max(v):8.1f} samples/s', flush=True)
        pv = rates['parent checkout']
        spread = (max(pv) - min(pv)) / med['parent checkout']
        ratio = med['this checkout'] / med['parent checkout']
        print(f'{wl:8s} this / parent = {ratio:.4f}; the parent against itself: (max - min) / median = {spread:.4f}; '
              f'{"within" if abs(ratio - 1.0) <= spread else "OUTSIDE"} that spread', flush=True)


if __name__ == '__main__':
    main()
