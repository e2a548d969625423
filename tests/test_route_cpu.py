"""mv2d_amd.route: the one place where the engine's option attributes become a route (which kernels run, which buffers they use).  Needs neither
the library nor a GPU."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from mv2d_amd import route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resolve(kind='S', exact=True, depth_num=64, map_dtype=torch.float32, keep_stages=False, use_graph=False, **options):
    opts = SimpleNamespace(**dict(route.default_options(), **options))
    return route.resolve(opts, kind, exact, depth_num, map_dtype, keep_stages, use_graph)


def test_route_module_needs_no_library():
    src = open(os.path.join(ROOT, 'mv2d_amd', 'route.py')).read()
    assert not re.search(r'^\s*(from|import)\s.*\b(ops|_lib)\b', src, re.M)


def test_every_switch_of_design_section_8_is_an_input_of_the_resolver():
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    sec8 = design[design.index('## 8. Switches'):]
    named = set(re.findall(r'`([a-z][a-z0-9_]*)`', sec8[sec8.index('Engine attributes'):]))
    assert {'lo8_rows', 'pe_at_positions', 'fuse_xattn', 'group_xattn', 'pe_rows_in_waves', 'fold_sa0', 'masked_transpose', 'exact_skip', 'fuse_maps',
            'q_order', 'xattn_waves', 'fork_qg', 'last_stage_heads', 'keep_sine_rows', 'force_nc', 'debug_attn'} <= named

    class Recorder:
        read = set()

        def __getattr__(self, name):
            self.read.add(name)
            return route.default_options()[name]
    route.resolve(Recorder(), 'S', True, 64)
    route.resolve(Recorder(), 'T', False, 64)               # (fork_qg only matters in key16 mode on the T path)
    assert named <= Recorder.read, named - Recorder.read
    assert Recorder.read == set(route.OPTIONS)              # ... and every default the engine sets is one the resolver reads


@pytest.mark.parametrize('kind', ['S', 'T'])
def test_default_routes_are_what_design_section_0_describes(kind):
    r = resolve(kind)
    assert r.exact and r.pe_x3 and r.attn_lo and r.lo8                 # index-exact: split-precision PE, hi + lo rows, the lo halves as e4m3 bytes
    assert not r.conv_x3                                               # the query generator's conv at single precision
    assert r.xattn_fused == (kind == 'S') and r.pe_at_pos == (kind == 'S') and r.pe_pos == (kind == 'S')
    assert r.q_order and r.fold_sa0 and r.masked and r.xattn_waves == 2 and r.fuse_maps is None
    assert not (r.grouped or r.group_tab or r.forked or r.stages or r.debug_attn or r.last_stage_heads or r.pe_rows_in_waves or r.keep_sine_rows
                or r.stop_before_decoder or r.ablate_zero_lo) and r.force_nc is None
    assert r.maps_fused(512) and not r.maps_fused(513)
    assert r.storage == (kind, True, True, kind == 'S', False, True) and r.storage._fields == ('kind', 'exact', 'lo8', 'pe_pos', 'group_tab', 'q_order')
    hash(r)                                                            # (part of the hipGraph key)


def test_key16_mode():
    r = resolve('T', exact=False)
    assert not (r.pe_x3 or r.conv_x3 or r.attn_lo or r.lo8 or r.pe_at_pos) and r.forked and not r.masked
    assert not resolve('T', exact=False, prof={}).forked and resolve('T', exact=False, prof={}, use_graph=True).forked
    assert not resolve('T', exact=False, fork_qg=False).forked and not resolve('S', exact=False).forked
    assert not resolve('S', exact=False).pe_pos


def test_derived_fields():
    assert not resolve('T', group_xattn=True).lo8 and resolve('T', group_xattn=True).grouped
    assert not resolve('S', keep_stages=True).pe_at_pos and resolve('S', keep_stages=True).pe_pos
    assert not resolve('S', exact_skip=frozenset({'pe'})).pe_at_pos
    r = resolve('S', keep_stages=True, last_stage_heads=True)
    assert r.stages and not r.last_stage_heads and not r.masked
    assert resolve('S', last_stage_heads=True).last_stage_heads
    d = resolve('S', debug_attn=True, group_xattn=True, fuse_maps=True)
    assert d.debug_attn and not d.grouped and not d.xattn_fused and not d.maps_fused(64) and d.group_tab
    assert not resolve('S', debug_attn=True, fuse_xattn=True).xattn_fused
    with pytest.raises(AssertionError, match='eager runs only'):
        resolve('S', debug_attn=True, use_graph=True)
    assert resolve('T', fuse_xattn=True).xattn_fused and not resolve('S', fuse_xattn=False).xattn_fused
    assert resolve('T', fuse_maps=False).maps_fused(64) is False and resolve('T', fuse_maps=True).maps_fused(4096)
    assert resolve('T', exact_skip=frozenset()).conv_x3 and not resolve('T', exact_skip=frozenset({'attn'})).attn_lo
    assert not resolve('T', keep_sine_rows=True).masked and not resolve('T', masked_transpose=False).masked


def test_denoising_route_of_the_training_forward():
    r = resolve('S').denoising()
    assert not (r.attn_lo or r.grouped or r.xattn_fused or r.q_order or r.fold_sa0 or r.debug_attn)
    assert resolve('S', fuse_xattn=True).denoising().xattn_fused
    assert r.last_stage_heads == resolve('S').last_stage_heads and r.xattn_waves == 2


def test_impossible_combinations_are_refused():
    with pytest.raises(ValueError, match='depth_num = 64 only'):
        resolve('S', exact=False, depth_num=48)
    with pytest.raises(ValueError, match=r'key16 mode\'s PE kernel \(csrc/pe_tab96.hip\)'):
        resolve('S', depth_num=48, exact_skip=frozenset({'pe'}))
    with pytest.raises(ValueError, match=r'pe_rows_in_waves \(csrc/pe_x3b.hip\) is built for depth_num = 64 only'):
        resolve('S', depth_num=48, pe_rows_in_waves=True)
    with pytest.raises(ValueError, match='pe_rows_in_waves.*reads fp32 feature maps only'):
        resolve('T', map_dtype=torch.float16, pe_rows_in_waves=True)
    with pytest.raises(ValueError, match='ablate_zero_lo works on key16 lo rows'):
        resolve('T', ablate_zero_lo=frozenset({'v'}))
    assert resolve('S', depth_num=48).pe_x3 and resolve('T', pe_rows_in_waves=True).pe_rows_in_waves
    assert resolve('T', ablate_zero_lo=frozenset({'v'}), lo8_rows=False).ablate_zero_lo == {'v'}
    assert resolve('T', exact=False, ablate_zero_lo=frozenset({'v'})).ablate_zero_lo == frozenset()       # (no lo rows to zero in key16 mode)


@pytest.mark.parametrize('kind', ['S', 'T'])
def test_launch_only_switches_share_storage_and_storage_switches_do_not(kind):
    base = resolve(kind)
    for option in (dict(last_stage_heads=True), dict(fuse_maps=False), dict(xattn_waves=4), dict(fold_sa0=False), dict(masked_transpose=False)):
        r = resolve(kind, **option)
        assert r.storage == base.storage and r != base, option
    assert resolve(kind, keep_stages=True).storage == base.storage and resolve(kind, keep_stages=True) != base
    assert resolve(kind, map_dtype=torch.float16).storage == base.storage and resolve(kind, map_dtype=torch.float16) != base
    for option in (dict(lo8_rows=False), dict(group_xattn=True), dict(q_order=False)) + ((dict(pe_at_positions=False),) if kind == 'S' else ()):
        assert resolve(kind, **option).storage != base.storage, option
    assert resolve(kind, exact=False).storage != base.storage and resolve('T').storage != resolve('S').storage
