#!/usr/bin/env python
"""What the decoder's shape (HeadEngine(num_layers=L, feedforward_channels=F)) costs next to the shipped 6 x 2048 (GPU only).

    python tools/bench_decoder_shape.py [--samples 16] [--rounds 3] [--shapes 6x2048,6x1024,...] [--root OTHER_CHECKOUT] [--eager]

Samples/s of ONE engine on ONE stream: run_batch of --samples samples per call, graph replay, for cfg2_s and cfg3_t at every shape of --shapes
(6x2048 = the shipped launches, the same run's yardstick), the shapes ALTERNATING inside one process; the median of --rounds rounds of 20 calls.
Not bench.py's number: that runs four streams with rotating inputs.

--root imports mv2d_amd from another checkout (an A/B of the shipped shape against another commit: run the two alternately, one process each; a
checkout from before the decoder shape keys takes only 6x2048).  --eager runs --calls eager launches per shape and problem and no timing (for a
kernel trace: rocprofv3 --kernel-trace --stats -- python tools/bench_decoder_shape.py --eager --calls 5; tools/rocpd_stats.py --by-grid then
separates the slab counts of one FFN instance)."""
import argparse
import os
import statistics
import sys
import time

DEFAULT_SHAPES = '6x2048,6x1024,3x2048,6x448,8x4096'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--shapes', default=DEFAULT_SHAPES)
    ap.add_argument('--problems', default='cfg2_s,cfg3_t')
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--label', default='')
    ap.add_argument('--eager', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch

    from mv2d_amd import synthetic
    from mv2d_amd.engine import HeadEngine
    dev = torch.device('cuda:0')
    B = args.samples
    shapes = [tuple(int(v) for v in s.split('x')) for s in args.shapes.split(',')]
    base = synthetic.make_head_state(seed=0)
    for name in args.problems.split(','):
        probs = [synthetic.make_problem(name, seed=s) for s in range(B)]
        feats = torch.cat([torch.from_numpy(p['feat']) for p in probs]).to(dev)
        props = [[torch.from_numpy(np.asarray(x)) for x in p['proposals']] for p in probs]
        metas = [p['img_metas'] for p in probs]
        kind, views = probs[0]['kind'], probs[0]['views_per_frame']
        engs = {}
        for L, F in shapes:
            if (L, F) == (6, 2048):
                engs[L, F] = HeadEngine(base, kind, dev, num_views=views)          # (no new argument: any checkout builds the shipped shape)
            else:
                engs[L, F] = HeadEngine(synthetic.with_decoder_shape_state(base, 0, L, F), kind, dev, num_views=views, num_layers=L,
                                        feedforward_channels=F)
        if args.eager:
            for (L, F), e in engs.items():
                for _ in range(args.calls):
                    e.results_batch(e.run_batch(feats, props, metas))
                print(f'{name} {L}x{F}: {args.calls} eager launches of {B} samples', flush=True)
            continue
        for e in engs.values():
            for _ in range(3):
                e.run_batch(feats, props, metas, use_graph=True)
        torch.cuda.synchronize()
        rates = {k: [] for k in engs}
        for _ in range(args.rounds):
            for k, e in engs.items():
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    e.run_batch(feats, props, metas, use_graph=True)
                torch.cuda.synchronize()
                rates[k].append(args.calls * B / (time.perf_counter() - t0))
        print(f'# {args.label}{name}: samples/s, one engine on one stream, run_batch of {B} samples, graph replay, median of {args.rounds} alternating '
              f'rounds of {args.calls} calls')
        for (L, F), v in rates.items():
            tag = ' (shipped launches)' if (L, F) == (6, 2048) else ''
            print(f'{args.label}{name} num_layers={L} feedforward_channels={F}{tag:19s} median {statistics.median(v):8.1f}   min {min(v):8.1f}   '
                  f'max {max(v):8.1f} samples/s', flush=True)


if __name__ == '__main__':
    main()
