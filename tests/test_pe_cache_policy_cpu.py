"""The host policy of the per-rig cache of the PE's frustum MLP (mv2d_amd/pe_cache.py, route option pe_cache): which frames build the table, which use
it, which run the full kernel.  Needs neither the library nor a GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mv2d_amd import pe_cache, route


def states(keys):
    pol = pe_cache.PeCachePolicy()
    return [pol.observe(k) for k in keys], pol


def test_a_repeated_key_builds_on_its_second_frame_and_hits_from_the_third():
    got, pol = states('AAA')
    assert got == ['miss', 'build', 'hit'] and pol.builds == 1
    assert states('AAAAA')[0] == ['miss', 'build', 'hit', 'hit', 'hit']


def test_alternating_keys_never_build():
    got, pol = states('ABAB')
    assert got == ['miss'] * 4 and pol.builds == 0
    got, pol = states([('rig', i) for i in range(6)])           # matrices that change every frame
    assert got == ['miss'] * 6 and pol.builds == 0


def test_one_entry_is_kept():
    got, pol = states('AABBA')
    assert got == ['miss', 'build', 'miss', 'build', 'miss'] and pol.builds == 2
    assert states('AABAA')[0] == ['miss', 'build', 'miss', 'miss', 'build']       # an old key that comes back: a miss, then a rebuild


def _mats(n_samples, views=2, seed=0):
    g = np.random.Generator(np.random.PCG64(seed))
    one = g.standard_normal((3, views, 4, 4))
    return np.concatenate([one] * n_samples, axis=1)


def test_a_weights_version_bump_is_a_miss():
    sk = (('geometry',),)
    a, b = pe_cache.rig_key(1, sk, 7), pe_cache.rig_key(2, sk, 7)
    assert a == pe_cache.rig_key(1, sk, 7) and a != b
    assert states([a, a, a, b, b, b])[0] == ['miss', 'build', 'hit', 'miss', 'build', 'hit']


def test_rig_key_follows_matrices_and_geometry():
    sk = (('geometry',),)
    a = pe_cache.rig_key(1, sk, 7)
    assert pe_cache.rig_key(1, sk, 8) != a                         # the engine's counter of matrix changes moved
    assert pe_cache.rig_key(1, (('other geometry',),), 7) != a
    hash(a)


def test_a_mixed_rig_batch_is_never_usable():
    sk = (('geometry',), ('geometry',))
    same = _mats(2)
    assert pe_cache.one_rig(same, 2) and pe_cache.one_rig(same[:, :2], 1)
    mixed = same.copy()
    mixed[1, 3, 2, 3] += 1e-9                                      # the second sample's second view: other extrinsics
    assert not pe_cache.one_rig(mixed, 2) and pe_cache.one_rig(mixed, 1)
    nan = same.copy()
    nan[0, 0, 0, 0] = nan[0, 2, 0, 0] = float('nan')               # (NaN matrices never compare equal)
    assert not pe_cache.one_rig(nan, 2)
    assert pe_cache.rig_key(1, sk, 7) == pe_cache.rig_key(1, sk[:1], 7) is not None              # the key of one of its samples alone
    assert pe_cache.rig_key(1, sk, 7, shared_rig=False) is None
    assert pe_cache.rig_key(1, (('geometry',), ('other geometry',)), 7) is None
    got, pol = states([None] * 4)
    assert got == ['miss'] * 4 and pol.builds == 0
    a = pe_cache.rig_key(1, sk, 7)
    assert states([a, a, None, a, a])[0] == ['miss', 'build', 'miss', 'miss', 'build']          # an unusable frame drops the table
    # what the engine does with a static batch of two rigs: the first frame is a miss whatever the rigs are, one_rig is asked when the matrices repeat
    assert states([a, None, None, None])[0] == ['miss'] * 4


def resolve(kind='S', exact=True, keep_stages=False, pe_options=None, **options):
    opts = SimpleNamespace(**dict(route.default_options(), **options))
    return route.resolve(opts, kind, exact, 64, torch.float32, keep_stages, False, pe_options=pe_options)


def test_the_route_allows_the_cache_where_the_gate_only_launch_can_stand_in():
    assert 'pe_cache' in route.OPTIONS and route.default_options()['pe_cache'] is True
    assert resolve('S').pe_cache and 'pe_cache' not in route.Storage._fields
    assert resolve('S').storage == resolve('S', pe_cache=False).storage and resolve('S') != resolve('S', pe_cache=False)
    for off in (dict(kind='T'), dict(exact=False), dict(keep_stages=True), dict(pe_cache=False), dict(keep_sine_rows=True), dict(pe_rows_in_waves=True),
                dict(exact_skip=frozenset({'pe'})), dict(pe_options=dict(with_fpe=False)), dict(pe_options=dict(no_sin_enc=True))):
        assert not resolve(**off).pe_cache, off
    assert resolve('S', pe_options=dict(with_fpe=True, no_sin_enc=False, LID=False)).pe_cache


def test_the_abi_test_of_the_repository_passes_with_the_new_entry():
    """tests/test_abi_cpu.py unchanged: the header declares mv2d_pe_gate_x3, the library exports it, _lib.SIGNATURES lists it, the ABI stays 6."""
    import test_abi_cpu as abi
    assert 'mv2d_pe_gate_x3' in abi.declared_functions()
    import __graft_entry__ as g
    g.build()
    from mv2d_amd import _lib
    lib = _lib.load()
    abi.test_header_symbols_are_exported(lib)
    abi.test_error_reporting_without_gpu(lib)
    rc = lib.mv2d_pe_gate_x3(None, None, None, None, 0, None, None, None, None, None, None, None, 1, None, None, None, None, None, 0, 0, None)
    assert rc == -1 and b'mv2d_pe_gate_x3' in lib.mv2d_last_error()
