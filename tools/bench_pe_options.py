#!/usr/bin/env python
"""What the PE's switches cost or save (GPU only): samples/s of one engine at the shipped PE, with_fpe=False and no_sin_enc=True, and the time of
the gate-less PE launch against the gated launch of the same library on the same rows.

    python tools/bench_pe_options.py [--samples 16] [--calls 20] [--runs 3] [--workloads cfg3_t cfg2_s]
    python tools/bench_pe_options.py --kernel [--workloads cfg3_t cfg2_s] [--launches 20]

Whole path: every (workload, variant) is measured in a child process of its own (one engine on one stream, run_batch of --samples samples, graph
replay, --calls calls per run), the median of --runs runs is reported; the children run one after the other, the variants alternating inside a
run.  Not bench.py's number: that runs four streams with rotating inputs.

--kernel: one process per workload.  A shipped engine runs one --samples launch with an fp32 and with an fp16 map; on its workspace (frustum rows,
feature map, key list, device-side row count, sine table: KS1 = 6) the PE launch of the engine (T path: key / value rows, S path: pe at the map
positions) is captured --launches times in a graph, gated (mv2d_pe_fused_x3 / _fmt) and gate-less (mv2d_pe_fused_x3_ng), alternating; the time per
launch is the median of --runs replays.  The gate-less kernel does strictly less work: a cell in which it is slower is reported as such and
the exit status is 1.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {'shipped': {}, 'with_fpe=False': dict(with_fpe=False), 'no_sin_enc=True': dict(no_sin_enc=True)}


def _setup(workload, samples, keys):
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from mv2d_amd import synthetic
    from mv2d_amd.engine import HeadEngine
    dev = torch.device('cuda:0')
    sd = synthetic.with_pe_options_state(synthetic.make_head_state(seed=0), keys.get('with_fpe', True), keys.get('no_sin_enc', False))
    probs = [synthetic.make_problem(workload, seed=s) for s in range(samples)]
    eng = HeadEngine(sd, probs[0]['kind'], dev, num_views=probs[0]['views_per_frame'], **keys)
    feats = torch.cat([torch.from_numpy(p['feat']) for p in probs]).to(dev)
    props = [[torch.from_numpy(np.asarray(x)) for x in p['proposals']] for p in probs]
    metas = [p['img_metas'] for p in probs]
    return torch, eng, feats, props, metas


def one(workload, variant, samples, calls):
    """Child mode: one JSON line with samples/s."""
    torch, eng, feats, props, metas = _setup(workload, samples, VARIANTS[variant])
    for _ in range(5):
        eng.run_batch(feats, props, metas, use_graph=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        eng.run_batch(feats, props, metas, use_graph=True)
    torch.cuda.synchronize()
    print(json.dumps(dict(workload=workload, variant=variant, samples_s=calls * samples / (time.perf_counter() - t0))), flush=True)


def kernel(workload, samples, launches, runs):
    """Child mode: the PE launch alone, gated against gate-less, on the rows of one --samples launch.  One JSON line per map format."""
    torch, eng, feats, props, metas = _setup(workload, samples, {})
    from mv2d_amd import ops
    for dt in (torch.float32, torch.float16):
        out = eng.run_batch(feats.to(dt), props, metas)
        torch.cuda.synchronize()
        ws = out['ws']
        rt, sh, P = ws['route'], ws['shared'], ws['P']
        S = int(ws['S_dev'].item())
        rows, at_pos = rt.kind == 'T', rt.pe_at_pos
        assert rt.pe_x3 and eng.pe_kp == 192

        def launch(gate):          # HeadEngine._exact_pe's call
            ops.pe_fused_x3(ws['xa1'], ws['featcl'], ws['S_dev'], eng.w['pe_x3'], sh['sine_tab'], sh['sine_period'],
                            pe=None if rows else (ws['pe_pos'] if at_pos else ws['pe']), Xk=(ws['Xk'], ws['xk_lo']) if rows else None,
                            Xv=(ws['Xf_b'], ws['xv_lo']) if rows else None, M=P, row_index=ws['s2pos'], pe_at_index=at_pos,
                            lo8_flag=ws['lo8_flag'] if (rows and rt.lo8) else None, **({} if gate else dict(gate=False, Kp=192)))
        graphs = {}
        for gate in (True, False):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                launch(gate)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode='thread_local'):
                for _ in range(launches):
                    launch(gate)
            g.replay()
            graphs[gate] = g
        torch.cuda.synchronize()
        us = {True: [], False: []}
        for _ in range(runs):
            for gate in (True, False):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[gate].replay()
                e1.record()
                e1.synchronize()
                us[gate].append(e0.elapsed_time(e1) * 1000.0 / launches)
        print(json.dumps(dict(workload=workload, map=str(dt).split('.')[-1], positions=P, rows=S, blocks=-(-S // 64), launches=launches,
                              gated_us=statistics.median(us[True]), nogate_us=statistics.median(us[False]),
                              gated_all=[round(v, 2) for v in us[True]], nogate_all=[round(v, 2) for v in us[False]])), flush=True)


def child(mode, args, timeout):
    cmd = [sys.executable, os.path.abspath(__file__)] + mode + ['--samples', str(args.samples), '--calls', str(args.calls), '--launches', str(args.launches),
                                                                 '--runs', str(args.runs)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        # a child that faulted, aborted or hung ends the measurement: nothing more is started on the device
        sys.exit(f'child {cmd} ended with status {r.returncode}:\n{r.stderr[-2000:]}')
    return [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith('{')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--one', nargs=2, metavar=('WORKLOAD', 'VARIANT'))
    ap.add_argument('--kernel-one', metavar='WORKLOAD')
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--workloads', nargs='+', default=['cfg3_t', 'cfg2_s'])
    ap.add_argument('--child-timeout', type=int, default=240)
    args = ap.parse_args()
    if args.one:
        return one(args.one[0], args.one[1], args.samples, args.calls)
    if args.kernel_one:
        return kernel(args.kernel_one, args.samples, args.launches, args.runs)
    if args.kernel:
        print(f'# the PE launch of one {args.samples}-sample run_batch, KS1 = 6, us per launch: {args.launches} launches per graph replay, median of {args.runs} '
              f'replays, gated and gate-less alternating (same library, same rows)')
        slower = 0
        for wl in args.workloads:
            for r in child(['--kernel-one', wl], args, args.child_timeout):
                ratio = r['nogate_us'] / r['gated_us']
                slower += ratio > 1.0
                print(f"{wl:8s} {r['map']:8s} map, {r['rows']:6d} rows of {r['positions']:6d} positions ({r['blocks']} blocks): gated {r['gated_us']:8.1f} us  "
                      f"gate-less {r['nogate_us']:8.1f} us  ratio {ratio:.3f} (k-steps: 56 / 72 = 0.778)   all: {r['gated_all']} / {r['nogate_all']}"
                      + ('   <-- GATE-LESS SLOWER' if ratio > 1.0 else ''), flush=True)
        return 1 if slower else 0
    print(f'# samples/s, one engine on one stream, run_batch of {args.samples} samples, graph replay, {args.calls} calls per run, median of {args.runs} runs '
          f'(one child process per run, variants alternating)')
    for wl in args.workloads:
        rates = {v: [] for v in VARIANTS}
        for _ in range(args.runs):
            for v in VARIANTS:
                rates[v].append(child(['--one', wl, v], args, args.child_timeout)[-1]['samples_s'])
        base = statistics.median(rates['shipped'])
        for v, x in rates.items():
            print(f'{wl:8s} {v:16s}: median {statistics.median(x):8.1f}   min {min(x):8.1f}   max {max(x):8.1f} samples/s   x {statistics.median(x) / base:.3f} of shipped', flush=True)


if __name__ == '__main__':
    sys.exit(main())
