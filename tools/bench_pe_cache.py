#!/usr/bin/env python
"""What the per-rig cache of the PE's frustum MLP (route option pe_cache, csrc/pe_x3_gate.hip) saves, and that a stream it cannot serve pays nothing
(GPU only).

    python tools/bench_pe_cache.py --kernel [--workload cfg2_s] [--samples 16] [--launches 20] [--runs 3]
    python tools/bench_pe_cache.py [--workload cfg2_s] [--moving] [--roots . ../parent] [--calls 20] [--runs 3]

--kernel: one process.  An engine runs a --samples batch three times (miss, build, hit); on its workspace (feature map, key list, device-side row
count, sine table, Q) the PE work of a frame is captured --launches times in a graph, as the full route runs it (mv2d_pe_frustum_f32 + mv2d_pe_fused_x3)
and as a hit runs it (mv2d_pe_gate_x3 alone), alternating; us per frame = the median of --runs replays.  The outputs of both forms are compared
bit for bit first.  Exit status 1 when the hit form takes more than half of the full one.

Whole path: samples/s of one engine on one stream (run_batch of --samples samples, graph replay, --calls calls per run, a child process per run),
for every tree in --roots (a checkout of another commit next to this one: the same script drives both) with pe_cache on and, in this tree, off;
the trees alternate inside a run.  --moving: the camera matrices differ on every frame (every call shifts the rig a little further), so no table
is ever built and every frame runs the full launches -- the stream the cache must cost nothing on.  Not bench.py's number (four streams).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup(root, workload, samples):
    sys.path.insert(0, os.path.abspath(root))
    import numpy as np
    import torch
    from mv2d_amd import synthetic
    from mv2d_amd.engine import HeadEngine
    dev = torch.device('cuda:0')
    probs = [synthetic.make_problem(workload, seed=s) for s in range(samples)]
    eng = HeadEngine(synthetic.make_head_state(seed=0), probs[0]['kind'], dev, num_views=probs[0]['views_per_frame'])
    feats = torch.cat([torch.from_numpy(p['feat']) for p in probs]).to(dev)
    props = [[torch.from_numpy(np.asarray(x)) for x in p['proposals']] for p in probs]
    metas = [p['img_metas'] for p in probs]
    return np, torch, eng, feats, props, metas


def _moved(np, metas, dx):
    out = []
    for m in metas:
        T = np.asarray(m['extrinsics']).T.copy()
        T[:3, 3] += [dx, 0.0, 0.0]
        out.append(dict(m, extrinsics=T.T.copy(), lidar2img=np.asarray(m['intrinsics']) @ T))
    return out


def one(root, workload, samples, calls, cache, moving):
    """Child mode: one JSON line with samples/s."""
    np, torch, eng, feats, props, metas = _setup(root, workload, samples)
    eng.pe_cache = bool(cache)
    pool = [[_moved(np, m, 0.001 * (j + 1)) for m in metas] for j in range(calls + 5)] if moving else None
    states = []
    for j in range(5):
        states.append(eng.run_batch(feats, props, pool[j] if moving else metas, use_graph=True).get('pe_cache'))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in range(calls):
        out = eng.run_batch(feats, props, pool[5 + j] if moving else metas, use_graph=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(workload=workload, root=root, cache=cache, moving=moving, samples_s=calls * samples / dt, warmup_states=states,
                          last_state=out.get('pe_cache'), builds=getattr(eng, 'pe_cache_builds', None))), flush=True)


def kernel(workload, samples, launches, runs):
    """Child mode: the PE work of one frame, full route against hit, on the rows of one --samples launch."""
    np, torch, eng, feats, props, metas = _setup(HERE, workload, samples)
    from mv2d_amd import ops
    for dt in (torch.float32, torch.float16):
        x = feats.to(dt)
        for want in ('miss', 'build', 'hit'):
            out = eng.run_batch(x, props, metas)
            assert out['pe_cache'] == want, (out['pe_cache'], want)
        torch.cuda.synchronize()
        ws = out['ws']
        rt, sh, P, T = ws['route'], ws['shared'], ws['P'], ws['tab']
        S = int(ws['S_dev'].item())
        V, h, w = ws['map_shape']
        assert rt.pe_x3 and rt.kind == 'S' and rt.pe_at_pos
        bufs = {form: torch.zeros_like(ws['pe_pos']) for form in ('full', 'hit')}

        def launch(form):          # HeadEngine._exact_pe's calls
            if form == 'full':
                ops.pe_frustum_f32(ws['s2pos'], ws['S_dev'], P, T['img2lidar'], T['coords_w'], T['coords_h'], T['coords_d'], ws['xa1'], V, h, w, eng.depth_num,
                                   eng.pe_range_h64, ld=eng.pe_kp)
                ops.pe_fused_x3(ws['xa1'], ws['featcl_cur'], ws['S_dev'], eng.w['pe_x3'], sh['sine_tab'], sh['sine_period'], pe=bufs[form], M=P, row_index=ws['s2pos'],
                                pe_at_index=True)
            else:
                ops.pe_gate_x3(sh['pe_q'], ws['featcl_cur'], ws['S_dev'], eng.w['pe_x3'], sh['sine_tab'], sh['sine_period'], bufs[form], P, row_index=ws['s2pos'],
                               pe_at_index=True)
        graphs = {}
        for form in bufs:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                launch(form)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode='thread_local'):
                for _ in range(launches):
                    launch(form)
            g.replay()
            graphs[form] = g
        torch.cuda.synchronize()
        equal = bool(torch.equal(bufs['full'], bufs['hit'])) and float(bufs['hit'].abs().sum()) > 0
        us = {form: [] for form in bufs}
        for _ in range(runs):
            for form in bufs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[form].replay()
                e1.record()
                e1.synchronize()
                us[form].append(e0.elapsed_time(e1) * 1000.0 / launches)
        print(json.dumps(dict(workload=workload, map=str(dt).split('.')[-1], positions=P, rows=S, blocks=-(-S // 64), launches=launches, bitwise_equal=equal,
                              full_us=statistics.median(us['full']), hit_us=statistics.median(us['hit']),
                              full_all=[round(v, 2) for v in us['full']], hit_all=[round(v, 2) for v in us['hit']])), flush=True)


def child(mode, args):
    cmd = [sys.executable, os.path.abspath(__file__)] + mode + ['--workload', args.workload, '--samples', str(args.samples), '--calls', str(args.calls),
                                                                 '--launches', str(args.launches), '--runs', str(args.runs)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
    if r.returncode != 0:
        # a child that faulted, aborted or hung ends the measurement: nothing more is started on the device
        sys.exit(f'child {cmd} ended with status {r.returncode}:\n{r.stderr[-2000:]}')
    return [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith('{')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--one', nargs=2, metavar=('ROOT', 'CACHE'))
    ap.add_argument('--kernel-one', action='store_true')
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--moving', action='store_true')
    ap.add_argument('--roots', nargs='+', default=[HERE])
    ap.add_argument('--workload', default='cfg2_s')
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--child-timeout', type=int, default=240)
    args = ap.parse_args()
    if args.one:
        return one(args.one[0], args.workload, args.samples, args.calls, int(args.one[1]), args.moving)
    if args.kernel_one:
        return kernel(args.workload, args.samples, args.launches, args.runs)
    if args.kernel:
        print(f'# the PE work of one {args.samples}-sample {args.workload} frame, us per frame: {args.launches} frames per graph replay, median of {args.runs} replays, '
              f'full route (pe_frustum_f32 + pe_x3) and hit (pe_x3_gate) alternating, one process')
        bad = 0
        for r in child(['--kernel-one'], args):
            ratio = r['hit_us'] / r['full_us']
            bad += ratio > 0.5 or not r['bitwise_equal']
            print(f"{args.workload:8s} {r['map']:8s} map, {r['rows']:6d} rows of {r['positions']:6d} positions ({r['blocks']} blocks): full {r['full_us']:8.1f} us  "
                  f"hit {r['hit_us']:8.1f} us  ratio {ratio:.3f} (bound 0.5; gate k-steps 16 / 72 = 0.222)   bitwise equal: {r['bitwise_equal']}   "
                  f"all: {r['full_all']} / {r['hit_all']}", flush=True)
        return 1 if bad else 0
    legs = [(root, 1) for root in args.roots] + [(HERE, 0)]
    print(f'# samples/s, one engine on one stream, run_batch of {args.samples} {args.workload} samples, graph replay, {args.calls} calls per run, {args.runs} runs '
          f'(one child process per run, legs alternating); matrices {"differ on every frame" if args.moving else "fixed"}')
    rates = {leg: [] for leg in legs}
    info = {}
    for _ in range(args.runs):
        for leg in legs:
            r = child(['--one', leg[0], str(leg[1])] + (['--moving'] if args.moving else []), args)[-1]
            rates[leg].append(r['samples_s'])
            info[leg] = (r['last_state'], r['builds'])
    for leg, x in rates.items():
        spread = (max(x) - min(x)) / statistics.median(x)
        print(f'{os.path.relpath(leg[0], HERE):12s} pe_cache={leg[1]}: median {statistics.median(x):8.1f}   min {min(x):8.1f}   max {max(x):8.1f} samples/s   spread '
              f'{100 * spread:.1f} %   last frame: {info[leg][0]}, tables built: {info[leg][1]}   all: {[round(v, 1) for v in x]}', flush=True)


if __name__ == '__main__':
    sys.exit(main())
