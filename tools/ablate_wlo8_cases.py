#!/usr/bin/env python
"""Would 8-BIT lo halves of the WEIGHT pairs keep the index-exact route index-exact?  Every split-precision kernel streams its weights from L2 as fp16
hi + lo pairs (4 B per weight); the lo half as e4m3 under a per-tensor power-of-two scale would make that 3 B.  Emulation of the storage format, kernels
unchanged: after the engine packed its weights, the lo tensors of the selected pairs are rounded through e4m3; then tests/test_gpu_golden.py's exact-mode
parity test runs on all of its (workload, seed) cases.
    python tools/ablate_wlo8_cases.py pe|maps|ffn|all [e4m3|e5m2]"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402
import test_gpu_golden as T  # noqa: E402

from mv2d_amd import ops  # noqa: E402
from mv2d_amd.engine import HeadEngine  # noqa: E402

scope = sys.argv[1] if len(sys.argv) > 1 else 'all'
fmt = torch.float8_e5m2 if (len(sys.argv) > 2 and sys.argv[2] == 'e5m2') else torch.float8_e4m3fn
PAT = {'pe': r'^pe_x3', 'maps': r'^ca_map', 'ffn': r'^ffn_w', 'all': r'.'}[scope]
FMAX = 448.0 if fmt == torch.float8_e4m3fn else 57344.0
init = HeadEngine.__init__
count = [0, 0]


def quantise(lo):
    m = float(lo.float().abs().max())
    if m == 0.0:
        return
    sc = 2.0 ** torch.floor(torch.log2(torch.tensor(FMAX / m))).item()
    lo.copy_(((lo.float() * sc).clamp(-FMAX, FMAX).to(fmt).float() / sc).to(lo.dtype))
    count[0] += 1
    count[1] += lo.numel()


def walk(name, v):
    q16 = ops.q16_dtype()
    if isinstance(v, dict):
        for k, x in v.items():
            walk(name + '.' + k, x)
    elif isinstance(v, (tuple, list)) and len(v) == 2 and all(torch.is_tensor(x) for x in v) and v[0].dtype == q16 and v[1].dtype == q16 and v[0].shape == v[1].shape:
        if re.search(PAT, name):
            quantise(v[1])


def patched(self, *a, **k):
    init(self, *a, **k)
    if self.exact:
        for key, v in self.w.items():
            walk(key, v)
        for i, table in enumerate(self.w['head_tables']):          # (class table, regression table): each starts with the hidden layers' (hi, lo) pair
            walk(f'head_tables.{i}', table[:2])


HeadEngine.__init__ = patched
cases = [m.args for m in T.test_exact_mode_integer_outputs_equal_the_reference.pytestmark if m.name == 'parametrize'][0][1]
bad = 0
for name, seed in cases:
    count[:] = [0, 0]
    try:
        T.test_exact_mode_integer_outputs_equal_the_reference(name, seed)
        print(f'    -> {name} seed {seed}: within the test bounds ({count[0]} lo tensors, {count[1]} weights rounded)')
    except AssertionError as e:
        bad += 1
        print(f'    -> {name} seed {seed}: FAILS the test bounds: {str(e)[:200]}')
print(f'{len(cases) - bad} of {len(cases)} cases pass with the lo halves of the {scope} weight pairs as {fmt}')
