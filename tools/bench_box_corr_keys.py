#!/usr/bin/env python
"""What the second instance of the correlation block costs: the fused frame-geometry launch, and the whole frame, at 128 (shipped), 576 and 4096
samples per (RoI, view) on a 16-sample cfg2_s batch (96 views, 4800 RoIs).

    python tools/bench_box_corr_keys.py [--out file.json]

Per key set: one engine, one stream.  (a) the launch alone: LAUNCHES calls of ops.frame_geometry on the batch's RoIs and matrices captured in one
graph, the replay timed with events, divided by LAUNCHES; (b) the frame: HeadEngine.run_batch(use_graph=True), REPLAYS replays timed with events.
Each figure is the median of three such timings after a warm-up.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mv2d_amd import calib, ops, synthetic  # noqa: E402
from mv2d_amd.engine import HeadEngine  # noqa: E402

# (sample_size, num_depth, depth_start, depth_end, LID)
KEY_SETS = ((4, 8, 0.5, 70, True), (6, 16, 0.3, 60, False), (8, 64, 0.5, 70, True))
BATCH, LAUNCHES, GRAPH_REPLAYS, REPLAYS = 16, 20, 20, 30


def timed(fn, n):
    """median of three: milliseconds per call of fn, n calls per timing"""
    out = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / n)
    return float(np.median(out)), [round(x, 4) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    probs = [synthetic.make_problem('cfg2_s', seed=i, with_feat=False) for i in range(BATCH)]
    V = probs[0]['views_per_frame']
    props = [[torch.from_numpy(p) for p in pr['proposals']] for pr in probs]
    metas = [pr['img_metas'] for pr in probs]
    g = torch.Generator(device=dev).manual_seed(0)
    feats = [torch.randn((V, 256, 32, 88), device=dev, generator=g) for _ in range(BATCH)]
    # ---- the batch as the engine lays it out: views numbered through, trans [B * V][V][16]
    rois, npv = [], []
    for b, pl in enumerate(props):
        for v, p in enumerate(pl):
            rois.append(torch.cat([torch.full((len(p), 1), float(b * V + v)), p[:, :4].float()], 1))
            npv.append(len(p))
    rois = torch.cat(rois).contiguous().to(dev)
    R = rois.shape[0]
    mats, _, trans, _ = calib.geometry_tables_batch(metas)
    viewK, viewE = (torch.from_numpy(mats[i]).reshape(BATCH * V, 16).contiguous().to(dev) for i in (0, 1))
    trans = trans.reshape(BATCH * V, V, 16).contiguous().to(dev)
    vs = torch.tensor(np.concatenate([[0], np.cumsum(npv)]), dtype=torch.int32, device=dev)
    pad_h, pad_w = metas[0][0]['pad_shape'][:2]
    intr, minv = torch.empty((R, 32), device=dev), torch.empty((R, 16), device=dev)
    match = torch.empty((R, V, 1), dtype=torch.int32, device=dev)
    zero = torch.empty((64 * 1024,), dtype=torch.uint8, device=dev)
    sd = synthetic.make_head_state(seed=0)
    res = dict(batch=BATCH, rois=R, views=BATCH * V, sets=[])
    for ss, D, ds, de, lid in KEY_SETS:
        t = calib.constant_tables(ss, D, ds, de, lid=lid)
        lin, depths = t['lin'].to(dev), t['depths'].to(dev)

        def launch():
            ops.frame_geometry(rois, viewK, viewE, intr, 32, minv, vs, trans, lin, depths, match, V, 1, int(pad_h), int(pad_w), max(npv), zero=zero,
                               sample_size=ss, num_depth=D, depth_start=ds)
        launch()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(LAUNCHES):
                launch()
        graph.replay()
        torch.cuda.synchronize()
        ms, raw = timed(graph.replay, GRAPH_REPLAYS)
        matched = int((match >= 0).sum())
        eng = HeadEngine(sd, 'S', dev, num_views=V, sample_size=ss, num_depth=D, corr_depth_start=ds, corr_depth_end=de, corr_LID=lid)
        for _ in range(3):
            eng.run_batch(feats, props, metas, use_graph=True)
        torch.cuda.synchronize()
        fms, fraw = timed(lambda: eng.run_batch(feats, props, metas, use_graph=True), REPLAYS)
        res['sets'].append(dict(sample_size=ss, num_depth=D, depth_start=ds, depth_end=de, LID=lid, samples=ss * ss * D, matched=matched,
                                frame_geometry_us=round(1e3 * ms / LAUNCHES, 2), frame_geometry_us_runs=[round(1e3 * x / LAUNCHES, 2) for x in raw],
                                frame_ms=round(fms, 4), frame_ms_runs=fraw))
        del eng
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
