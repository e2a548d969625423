#!/usr/bin/env python
"""What the per-view cache of the PE's frustum MLP (route option pe_cache_views, two-frame head) does to a stream whose current-frame views repeat
their matrices while the previous-frame views carry the ego motion (GPU only).

    python tools/bench_pe_cache_views.py [--workload cfg3_t] [--samples 16] [--sets 4] [--calls 40] [--runs 3]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_pe_cache_views.py --one 1        (the PE launches' times: a run of its own)

One engine on one stream, run_batch of --samples samples, graph replay.  --sets frame sets share the current-frame matrices and differ in `ego`
(synthetic.make_img_metas: the previous-frame views' extrinsics and time stamps); the calls rotate through them, so on every call the current-frame
views hit their slices and the previous-frame views run the full kernel.  Option off and on alternate, one child process per run, --runs runs each;
samples/s = median, with min / max.  Each child also reports the share of the key rows that lay in cached views.  Not bench.py's number (four streams).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(workload, samples, sets, calls, option):
    """Child mode: one JSON line."""
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from mv2d_amd import synthetic
    from mv2d_amd.engine import HeadEngine
    dev = torch.device('cuda:0')
    probs = [synthetic.make_problem(workload, seed=s) for s in range(samples)]
    assert probs[0]['kind'] == 'T' and probs[0]['frames'] == 2, 'a two-frame workload'
    eng = HeadEngine(synthetic.make_head_state(seed=0), 'T', dev, num_views=probs[0]['views_per_frame'])
    eng.pe_cache_views = bool(option)
    feats = torch.cat([torch.from_numpy(p['feat']) for p in probs]).to(dev)
    props = [[torch.from_numpy(np.asarray(x)) for x in p['proposals']] for p in probs]
    metas = [[synthetic.make_problem(workload, seed=0, with_feat=False, ego=0.05 * (j + 1))['img_metas']] * samples for j in range(sets)]
    states = []
    for j in range(2 * sets):
        states.append(eng.run_batch(feats, props, metas[j % sets], use_graph=True)['pe_cache'])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in range(calls):
        out = eng.run_batch(feats, props, metas[j % sets], use_graph=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ws = out['ws']
    S = int(ws['S_dev'].item())
    V, h, w = ws['map_shape']
    view = (ws['s2pos'][:S].long() % ((V // samples) * h * w)) // (h * w)
    cached = torch.zeros(S, dtype=torch.bool, device=dev)
    for v in out.get('pe_cache_views', ()):
        cached |= view == v
    print(json.dumps(dict(workload=workload, option=option, samples_s=calls * samples / dt, warmup_states=states, last_state=out['pe_cache'],
                          views=list(out.get('pe_cache_views', ())), rows=S, blocks=-(-S // 64), cached_rows=int(cached.sum()),
                          builds=getattr(eng, 'pe_cache_builds', 0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--one', type=int, default=None, metavar='OPTION')
    ap.add_argument('--workload', default='cfg3_t')
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--sets', type=int, default=4)
    ap.add_argument('--calls', type=int, default=40)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--child-timeout', type=int, default=240)
    args = ap.parse_args()
    if args.one is not None:
        return one(args.workload, args.samples, args.sets, args.calls, args.one)
    print(f'# samples/s, one engine on one stream, run_batch of {args.samples} {args.workload} samples, graph replay, {args.calls} calls per run rotating through '
          f'{args.sets} frame sets (same current-frame matrices, other ego), {args.runs} runs per leg (one child process per run, legs alternating)')
    rates, info = {0: [], 1: []}, {}
    for _ in range(args.runs):
        for option in (0, 1):
            cmd = [sys.executable, os.path.abspath(__file__), '--one', str(option), '--workload', args.workload, '--samples', str(args.samples),
                   '--sets', str(args.sets), '--calls', str(args.calls)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            if r.returncode != 0:
                # a child that faulted, aborted or hung ends the measurement: nothing more is started on the device
                sys.exit(f'child {cmd} ended with status {r.returncode}:\n{r.stderr[-2000:]}')
            res = [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith('{')][-1]
            rates[option].append(res['samples_s'])
            info[option] = res
    for option, x in rates.items():
        i = info[option]
        spread = (max(x) - min(x)) / statistics.median(x)
        print(f'pe_cache_views={option}: median {statistics.median(x):8.1f}   min {min(x):8.1f}   max {max(x):8.1f} samples/s   spread {100 * spread:.1f} %   '
              f'last frame: {i["last_state"]}, cached views {i["views"]}, {i["cached_rows"]} of {i["rows"]} key rows ({100.0 * i["cached_rows"] / max(i["rows"], 1):.1f} %) in '
              f'cached views, {i["blocks"]} row tiles, builds {i["builds"]}   all: {[round(v, 1) for v in x]}', flush=True)
    print(f'# ratio of medians on / off: {statistics.median(rates[1]) / statistics.median(rates[0]):.3f}')


if __name__ == '__main__':
    sys.exit(main())
