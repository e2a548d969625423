#!/usr/bin/env python
"""Replay the head engine's hipGraph a few times on one stream (a profiling target for tools/prof_cmd.sh):
    python tools/run_engine.py --workload cfg2_s --batch 8 --steps 20 [--exact] [--eager] [--num-classes N] [--roi-size S]
        [--feat-dtype fp32|fp16|bf16] [--upcast]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mv2d_amd import synthetic  # noqa: E402
from mv2d_amd.engine import HeadEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--workload', default='cfg2_s')
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--exact', action='store_true', help='(the default since round 5; accepted and ignored)')
ap.add_argument('--key16', action='store_true', help='the opt-in key16 mode (one fp16 rounding of the key side)')
ap.add_argument('--eager', action='store_true')
ap.add_argument('--pe-v2', action='store_true', help='the opt-in second shape of the PE kernel (csrc/pe_x3b.hip) instead of csrc/pe_x3.hip')
ap.add_argument('--group', type=int, default=None, help='1 / 0: force the shared-tile cross attention (csrc/xattn_group.hip) on / off; default: the engine chooses (T path: on)')
ap.add_argument('--num-classes', type=int, default=10, help='class count of the head (synthetic weights of that many classes)')
ap.add_argument('--roi-size', type=int, default=7, help='RoIAlign output size s (s x s bins, 1..14; the weights do not depend on it)')
ap.add_argument('--feat-dtype', choices=('fp32', 'fp16', 'bf16'), default='fp32', help='dtype of the feature map handed to the engine (16-bit maps are read natively)')
ap.add_argument('--upcast', action='store_true', help='with a 16-bit --feat-dtype: cast the map to fp32 with torch in front of every call (what a caller had to do before the engine took 16-bit maps)')
a = ap.parse_args()
dev = torch.device('cuda:0')
probs = [synthetic.make_problem(a.workload, seed=s) for s in range(a.batch)]
eng = HeadEngine(synthetic.make_head_state(seed=0, num_classes=a.num_classes), probs[0]['kind'], dev, num_views=probs[0]['views_per_frame'],
                 exact=not a.key16, num_classes=a.num_classes, roi_size=a.roi_size)
eng.fork_qg = False
if a.pe_v2:
    eng.pe_rows_in_waves = True
if a.group is not None:
    eng.group_xattn = bool(a.group)
feats = torch.cat([torch.from_numpy(p['feat']) for p in probs]).to(dev).to({'fp32': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}[a.feat_dtype])
feat_in = (lambda: feats.float()) if a.upcast else (lambda: feats)
props = [[torch.from_numpy(x) for x in p['proposals']] for p in probs]
metas = [p['img_metas'] for p in probs]
run = (lambda: eng.run_batch(feat_in(), props, metas, use_graph=not a.eager)) if a.batch > 1 else (lambda: eng.run(feat_in(), props[0], metas[0], use_graph=not a.eager))
for _ in range(3):
    run()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(a.steps):
    run()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / a.steps
print(f'{a.workload} batch {a.batch} num_classes {a.num_classes} roi_size {a.roi_size} feat {a.feat_dtype + (" upcast by torch" if a.upcast else "")} route={"key16" if a.key16 else "index-exact"}: {dt * 1e3:.3f} ms per launch sequence, {a.batch / dt:.0f} samples/s on one stream')
