#!/usr/bin/env python
"""What the RegLayer regression branches (HeadEngine(use_reg_layer=True)) cost next to the shipped branches (GPU only).

    python tools/bench_reg_layer.py [--samples 16] [--rounds 30]

1. Launch times at the rows of cfg2_s with --samples samples per launch (R = 300 each): today's one launch mv2d_heads_depth_x3 against the
   pair mv2d_heads_cls_depth_x3 + mv2d_reg_layer_depth_x3 (n = 2, on the engines' own tables), each as a captured graph of 20 launches, the
   variants ALTERNATING inside one process (median and minimum over --rounds rounds).
2. Samples/s of one engine on one stream (run_batch of --samples cfg2_s samples, graph replay) with the switch off and on, alternating.
   Not bench.py's number: that runs four streams with rotating inputs."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mv2d_amd import ops, synthetic  # noqa: E402
from mv2d_amd.engine import HeadEngine  # noqa: E402

DEV = torch.device('cuda:0')
DIMS = (2, 2, 1, 1, 2, 2)


def graph_of(fn, n=20):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g, n


def time_graph(g, n, reps=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (n * reps) * 1e3          # us per call of fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=30)
    args = ap.parse_args()
    L, M = 6, 300 * args.samples
    sd = synthetic.make_head_state(seed=0)
    sd_rl = synthetic.with_reg_layer_state(sd, 0, DIMS)
    prob = synthetic.make_problem('cfg2_s', seed=0)
    plain = HeadEngine(sd, 'S', DEV, num_views=prob['views_per_frame'])
    regl = HeadEngine(sd_rl, 'S', DEV, num_views=prob['views_per_frame'], use_reg_layer=True, group_reg_dims=DIMS)
    g = torch.Generator().manual_seed(1)
    outs, ref = torch.randn((L, M, 256), generator=g).to(DEV), torch.rand((M, 3), generator=g).to(DEV)
    cls, reg = torch.empty((L, M, 10), device=DEV), torch.empty((L, M, 10), device=DEV)
    pcr = plain.pc_range_h
    variants = {
        'heads_depth_x3 (cls + Sequential reg, one launch)': lambda: ops.heads_depth_x3(outs, plain.cls_ptrs_x3, plain.reg_ptrs_x3, ref, cls, reg, M, L, 2, pcr),
        'heads_cls_depth_x3 (cls alone)': lambda: ops.heads_cls_depth_x3(outs, regl.cls_ptrs_x3, cls, M, L, 2),
        'reg_layer_depth_x3 (RegLayer reg alone)': lambda: ops.reg_layer_depth_x3(outs, regl.reg_ptrs_x3, ref, reg, M, L, 2, DIMS, pcr),
        'heads_cls_depth_x3 + reg_layer_depth_x3 (the pair)': lambda: (ops.heads_cls_depth_x3(outs, regl.cls_ptrs_x3, cls, M, L, 2),
                                                                       ops.reg_layer_depth_x3(outs, regl.reg_ptrs_x3, ref, reg, M, L, 2, DIMS, pcr)),
    }
    graphs = {k: graph_of(fn) for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, (gr, n) in graphs.items():
            times[k].append(time_graph(gr, n))
    print(f'# launch times, L = {L} layers, M = {M} rows ({args.samples} cfg2_s samples per launch), {args.rounds} alternating rounds of 100 launches')
    for k, v in times.items():
        print(f'{k:52s} median {statistics.median(v):8.1f} us   min {min(v):8.1f} us')

    # ---- one engine, one stream, graph replay
    B = args.samples
    probs = [synthetic.make_problem('cfg2_s', seed=s) for s in range(B)]
    feats = torch.cat([torch.from_numpy(p['feat']) for p in probs]).to(DEV)
    props = [[torch.from_numpy(np.asarray(x)) for x in p['proposals']] for p in probs]
    metas = [p['img_metas'] for p in probs]
    rates = {'use_reg_layer=False': [], 'use_reg_layer=True': []}
    engs = {'use_reg_layer=False': plain, 'use_reg_layer=True': regl}
    for e in engs.values():
        for _ in range(5):
            e.run_batch(feats, props, metas, use_graph=True)
    torch.cuda.synchronize()
    for _ in range(6):
        for k, e in engs.items():
            t0 = time.perf_counter()
            for _ in range(20):
                e.run_batch(feats, props, metas, use_graph=True)
            torch.cuda.synchronize()
            rates[k].append(20 * B / (time.perf_counter() - t0))
    print(f'# samples/s, one engine on one stream, run_batch of {B} cfg2_s samples, graph replay, 6 alternating rounds of 20 calls')
    for k, v in rates.items():
        print(f'{k:52s} median {statistics.median(v):8.1f}   max {max(v):8.1f} samples/s')


if __name__ == '__main__':
    main()
