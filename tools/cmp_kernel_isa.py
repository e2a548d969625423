#!/usr/bin/env python
"""Are the instruction streams of a source file's kernels what they were at another commit?

    python tools/cmp_kernel_isa.py [--work-classes] <git-rev> rows.hip geometry.hip pe_x3.hip pe_tab96.hip

Compiles mv2d_amd/csrc/<file> of <git-rev> and of the working tree for gfx950 (device code only, the flags of mv2d_amd/build.py), disassembles both code
objects with llvm-objdump -d and compares kernel by kernel.  A kernel that gained a template argument is matched with its `float` instance
(`roi_align_kernel` <-> `roi_align_kernel<float>`, `pe_inputs_kernel<true>` <-> `pe_inputs_kernel<true, float>`).  No GPU needed.  Exit status 1
when a kernel of <git-rev> is missing or differs.

--work-classes: for code that moved between functions, where the compiler re-numbers registers and re-pairs scalar arithmetic.  A kernel that
differs gets its old and new instruction counts per opcode prefix printed, and passes when the counts of the WORK classes are equal: MFMAs, global
loads and stores, LDS instructions, v_exp / v_rcp / v_perm / v_cvt, barriers and every DPP instruction.  (Two v_mul_f32 that became one
v_pk_mul_f32 give the same bits; an MFMA, a load or a conversion more or less does not.)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mv2d_amd.build import FLAGS, _hipcc  # noqa: E402

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
ZERO_DWORD = 'v_cndmask_b32_e32 v0, s0, v0, vcc'             # what llvm-objdump makes of 0x00000000


def kernels(src, tmp, tag):
    bundle, co = os.path.join(tmp, tag + '.bundle'), os.path.join(tmp, tag + '.co')
    subprocess.run([_hipcc()] + FLAGS + ['--cuda-device-only', '-c', src, '-o', bundle], check=True)
    subprocess.run([os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950',
                    '--input=' + bundle, '--output=' + co], check=True)
    txt = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        ins = line.split('//')[0].strip()
        if cur is None or not ins or ins == '...':           # (padding behind s_endpgm)
            continue
        cur.append(re.sub(r'<[^>]+>', '<sym>', ins))
    for ins in out.values():             # (one dword of zero padding behind the last s_endpgm is printed as an instruction, not as `...`; whether it
        end = max((i for i, s in enumerate(ins) if s == 's_endpgm'), default=len(ins) - 1)       # is there depends on where the next kernel starts)
        if all(s == ZERO_DWORD for s in ins[end + 1:]):
            del ins[end + 1:]
    names = subprocess.run(['c++filt'], input='\n'.join(out), capture_output=True, text=True, check=True).stdout.split('\n')
    res = {}
    for mangled, name in zip(out, names):
        name = name.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0].replace('> >', '>>')
        name = name[:-len(' [clone .kd]')] if name.endswith(' [clone .kd]') else name
        res[name] = out[mangled]
    return res


WORK = ('v_mfma', 'global_load', 'global_store', 'ds_', 'v_exp', 'v_rcp', 'v_perm', 'v_cvt', 's_barrier')


def classes(ins):
    """instruction count per opcode prefix: the work classes by their names, `*_dpp`, everything else by its first two words (v_mul, s_add, ...)"""
    out = {}
    for i in ins:
        op = i.split()[0]
        key = next((w for w in WORK if op.startswith(w)), None) or ('*_dpp' if op.endswith('_dpp') else '_'.join(op.split('_')[:2]))
        out[key] = out.get(key, 0) + 1
    return out


def work_equal(old, new, label):
    a, b = classes(old), classes(new)
    same = True
    for key in sorted(set(a) | set(b)):
        work = key in WORK or key == '*_dpp'
        if a.get(key, 0) != b.get(key, 0):
            print('    %-14s %6d -> %6d%s' % (key, a.get(key, 0), b.get(key, 0), '   <-- WORK CLASS' if work else ''))
            same = same and not work
        elif work:
            print('    %-14s %6d    %6d' % (key, a[key], b[key]))
    return same


def main():
    args = sys.argv[1:]
    by_class = '--work-classes' in args
    args = [a for a in args if a != '--work-classes']
    rev, files = args[0], args[1:]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, 'old')
        os.makedirs(old)
        tar = subprocess.run(['git', '-C', ROOT, 'archive', rev, 'mv2d_amd/csrc'], check=True, capture_output=True).stdout
        subprocess.run(['tar', '-x', '-C', old], input=tar, check=True)
        for f in files:
            a = kernels(os.path.join(old, 'mv2d_amd', 'csrc', f), tmp, 'old_' + f)
            b = kernels(os.path.join(ROOT, 'mv2d_amd', 'csrc', f), tmp, 'new_' + f)
            for name, ins in sorted(a.items()):
                cands = [name, name + '<float>', re.sub(r'>$', ', float>', name)]
                now = next((c for c in cands if c in b), None)
                verdict = 'MISSING' if now is None else ('identical' if b[now] == ins else 'DIFFERENT (%d -> %d instructions)' % (len(ins), len(b[now])))
                print('%-14s %-78s %6d  %s' % (f, (now or name)[:78], len(ins), verdict))
                if by_class and verdict.startswith('DIFFERENT'):
                    ok = work_equal(ins, b[now], now)
                    print('    -> work classes %s' % ('equal' if ok else 'DIFFER'))
                    bad += not ok
                else:
                    bad += verdict != 'identical'
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
