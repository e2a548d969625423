"""The host policy of the PER-VIEW cache of the PE's frustum MLP on the two-frame head (mv2d_amd/pe_cache.py PeViewCachePolicy / view_keys, route option
pe_cache_views): which views' slices a frame builds, which it reads, which rows run the full kernel.  Needs neither a GPU nor (but for the ABI test) the
library."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mv2d_amd import pe_cache, route

SK = (('geometry',),)


def mats(cur=0.0, prev=0.0, n_samples=1, views=4):
    """[3 kinds, n_samples * views, 4, 4]: views 0 .. views/2 - 1 are the current frame (moved by `cur`), the others the previous frame (moved by `prev`)"""
    g = np.random.Generator(np.random.PCG64(3))
    one = g.standard_normal((3, views, 4, 4))
    one[:, :views // 2, 0, 3] += cur
    one[:, views // 2:, 0, 3] += prev
    return np.concatenate([one] * n_samples, axis=1)


def run(frames, n_samples=1, views=4, version=1, sk=SK):
    pol = pe_cache.PeViewCachePolicy(views)
    return [pol.observe(pe_cache.view_keys(version, sk * n_samples, m, n_samples)) for m in frames], pol


def test_current_views_repeat_while_previous_views_move():
    got, pol = run([mats(prev=e) for e in (0.0, 0.1, 0.2, 0.3)])
    assert got == [(0, (), 'miss'), (0b0011, (0, 1), 'build'), (0b0011, (), 'hit'), (0b0011, (), 'hit')] and pol.builds == 1
    assert pe_cache.mask_views(0b0011) == (0, 1) and pe_cache.mask_views(0) == () and pe_cache.mask_views(1 << 31) == (31,)


def test_all_views_repeat():
    got, pol = run([mats()] * 4)
    assert got == [(0, (), 'miss'), (0b1111, (0, 1, 2, 3), 'build'), (0b1111, (), 'hit'), (0b1111, (), 'hit')] and pol.builds == 1
    # the previous-frame views come to rest later: their slices are built beside the held ones
    got, pol = run([mats(prev=e) for e in (0.0, 0.1, 0.2, 0.2, 0.2)])
    assert got[2:] == [(0b0011, (), 'hit'), (0b1111, (2, 3), 'build'), (0b1111, (), 'hit')] and pol.builds == 2


def test_a_changed_view_drops_only_its_own_slice():
    a, b = mats(), mats()
    b[2, 1, 1, 1] += 1e-9                               # view 1: another lidar2img
    got, _ = run([a, a, a, b, b, b])
    assert got == [(0, (), 'miss'), (0b1111, (0, 1, 2, 3), 'build'), (0b1111, (), 'hit'), (0b1101, (), 'hit'), (0b1111, (1,), 'build'), (0b1111, (), 'hit')]
    got, _ = run([a, a, mats(cur=1.0, prev=1.0)])       # the whole rig shifted
    assert got[-1] == (0, (), 'miss')
    got, _ = run([a, a, b, a, a])                       # an old key that comes back: a miss of that view, then a rebuild
    assert got[2:] == [(0b1101, (), 'hit'), (0b1101, (), 'hit'), (0b1111, (1,), 'build')]


def test_a_view_in_which_the_samples_differ_stays_uncached():
    same = mats(n_samples=2)
    assert all(k is not None for k in pe_cache.view_keys(1, SK * 2, same, 2))
    assert pe_cache.view_keys(1, SK * 2, same, 2) == pe_cache.view_keys(1, SK, same[:, :4], 1)      # the keys of one of its samples alone
    mixed = same.copy()
    mixed[1, 4 + 1, 2, 3] += 1e-9                       # the second sample's view 1: other extrinsics
    keys = pe_cache.view_keys(1, SK * 2, mixed, 2)
    assert [k is None for k in keys] == [False, True, False, False]
    got, pol = run([mixed] * 3, n_samples=2)
    assert got == [(0, (), 'miss'), (0b1101, (0, 2, 3), 'build'), (0b1101, (), 'hit')]
    nan = same.copy()
    nan[0, 0, 0, 0] = nan[0, 4, 0, 0] = float('nan')    # (NaN matrices never compare equal)
    assert pe_cache.view_keys(1, SK * 2, nan, 2)[0] is None
    # samples of different padding geometry: no view is usable
    assert pe_cache.view_keys(1, (('geometry',), ('other geometry',)), same, 2) == [None] * 4
    pol = pe_cache.PeViewCachePolicy(4)
    assert [pol.observe(pe_cache.view_keys(1, (('geometry',), ('other geometry',)), same, 2)) for _ in range(3)] == [(0, (), 'miss')] * 3 and pol.builds == 0


def test_new_weights_and_new_geometry_rebuild():
    pol = pe_cache.PeViewCachePolicy(4)
    m = mats()
    seq = [pol.observe(pe_cache.view_keys(v, sk, m, 1)) for v, sk in ((1, SK), (1, SK), (1, SK), (2, SK), (2, SK), (2, (('other',),)), (2, (('other',),)))]
    assert [s[2] for s in seq] == ['miss', 'build', 'hit', 'miss', 'build', 'miss', 'build'] and pol.builds == 3
    assert seq[3] == (0, (), 'miss') and seq[4][1] == (0, 1, 2, 3)
    hash(pe_cache.view_keys(1, SK, m, 1)[0])


def test_an_unusable_frame_drops_every_slice():
    pol = pe_cache.PeViewCachePolicy(2)
    k = pe_cache.view_keys(1, SK, mats(views=2), 1)
    assert [pol.observe(x)[2] for x in (k, k, [None, None], k, k)] == ['miss', 'build', 'miss', 'miss', 'build']
    with pytest.raises(ValueError, match='2 views'):
        pol.observe(k + k)
    with pytest.raises(ValueError, match='1 to 32 views'):
        pe_cache.PeViewCachePolicy(33)
    assert pe_cache.PeViewCachePolicy(32).observe([('k', v) for v in range(32)]) == (0, (), 'miss')


def resolve(kind='T', exact=True, keep_stages=False, pe_options=None, **options):
    opts = SimpleNamespace(**dict(route.default_options(), **options))
    return route.resolve(opts, kind, exact, 64, torch.float32, keep_stages, False, pe_options=pe_options)


def test_the_option_is_off_by_default_and_the_environment_turns_it_on(monkeypatch):
    assert 'pe_cache_views' in route.OPTIONS and route.default_options()['pe_cache_views'] is False
    assert not resolve('T').pe_cache_views and not resolve('S').pe_cache_views
    monkeypatch.setenv('MV2D_PE_CACHE_VIEWS', '1')
    assert route.default_options()['pe_cache_views'] is True
    monkeypatch.setenv('MV2D_PE_CACHE_VIEWS', '0')
    assert route.default_options()['pe_cache_views'] is False


def test_the_route_allows_the_per_view_cache_where_the_split_launches_can_stand_in():
    on = dict(pe_cache_views=True)
    assert resolve('T', **on).pe_cache_views and 'pe_cache_views' not in route.Storage._fields
    assert resolve('T', **on).storage == resolve('T').storage and resolve('T', **on) != resolve('T')          # (the route is part of the graph key)
    for off in (dict(kind='S'), dict(exact=False), dict(keep_stages=True), dict(keep_sine_rows=True), dict(pe_rows_in_waves=True),
                dict(exact_skip=frozenset({'pe'})), dict(pe_options=dict(with_fpe=False)), dict(pe_options=dict(no_sin_enc=True))):
        assert not resolve(**dict(dict(kind='T'), **off), **on).pe_cache_views, off
    assert resolve('T', pe_options=dict(with_fpe=True, no_sin_enc=False, LID=False), **on).pe_cache_views
    # the S path ignores the option and keeps pe_cache as it is; the T path never had pe_cache
    assert resolve('S', **on) == resolve('S')._replace(pe_cache_views=False) and resolve('S', **on).pe_cache
    assert not resolve('T', **on).pe_cache and resolve('T', pe_cache=False, **on).pe_cache_views


def test_every_option_is_read_by_the_resolver():
    """the rule of tests/test_route_cpu.py's Recorder with the new option in the list"""
    class Recorder:
        read = set()

        def __getattr__(self, name):
            self.read.add(name)
            return route.default_options()[name]
    route.resolve(Recorder(), 'S', True, 64)
    route.resolve(Recorder(), 'T', False, 64)
    assert 'pe_cache_views' in Recorder.read and Recorder.read == set(route.OPTIONS)


def test_the_library_exports_the_new_entries_and_they_refuse_by_name():
    """the header declares the three entries, the library exports them, _lib.SIGNATURES lists them position by position, the ABI stays 6; without a view
    mask (or with more than 32 views, or a period that is no multiple of hw) each refuses and names itself -- no GPU touched"""
    import test_abi_cpu as abi
    new = ('mv2d_pe_gate_rows_x3', 'mv2d_pe_fused_x3_k_sel', 'mv2d_pe_frustum_f32_sel')
    assert set(new) <= set(abi.declared_functions())
    import __graft_entry__ as g
    g.build()
    from mv2d_amd import _lib
    lib = _lib.load()
    assert set(new) <= set(_lib.SIGNATURES)
    abi.test_header_symbols_are_exported(lib)
    abi.test_signatures_agree_with_the_header_position_by_position()
    abi.test_error_reporting_without_gpu(lib)
    import ctypes
    one = ctypes.addressof(ctypes.create_string_buffer(4096))
    # (Q | A1, Xmap, row_index, m_dev, M, weights ..., sine_tab, tab_period, pe, four rows, lo_fmt, lo8_flag, map_fmt, [Kp,] view_mask, hw, take_set, stream)
    gate = lambda mask, hw, period: lib.mv2d_pe_gate_rows_x3(one, one, None, None, 4, *([one] * 7), period, None, one, one, one, one, 0, None, 0, mask, hw, 1, None)  # noqa: E731
    full = lambda mask, hw, period: lib.mv2d_pe_fused_x3_k_sel(one, one, None, None, 4, *([one] * 13), period, None, one, one, one, one, 0, None, 0, 192,  # noqa: E731
                                                               mask, hw, 0, None)
    frus = lambda mask, hw, period: lib.mv2d_pe_frustum_f32_sel(one, one, 4, one, one, one, one, one, 4, hw, 1, 64, one, 192, mask, period, None)  # noqa: E731
    for fn, name in ((gate, new[0]), (full, new[1]), (frus, new[2])):
        for args in ((None, 48, 192), (one, 48, 200), (one, 48, 48 * 33), (one, 0, 192)):
            assert fn(*args) == -1 and name.encode() in lib.mv2d_last_error(), (name, args, lib.mv2d_last_error())
    assert lib.mv2d_pe_gate_rows_x3(one, one, None, None, 4, *([one] * 7), 192, None, None, one, one, one, 0, None, 0, one, 48, 1, None) == -1
    assert b'mv2d_pe_gate_rows_x3' in lib.mv2d_last_error() and b'row outputs' in lib.mv2d_last_error()
    assert lib.mv2d_pe_fused_x3_k_sel(one, one, None, None, 4, *([one] * 13), 192, None, one, one, one, one, 0, None, 0, 100, one, 48, 0, None) == -1
    assert b'mv2d_pe_fused_x3_k_sel: Kp' in lib.mv2d_last_error()
