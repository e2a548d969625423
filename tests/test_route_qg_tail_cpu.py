"""Route field qg_tail_fused (option fuse_qg_tail): on by default, off for keep_stages runs and when switched off; launch-only."""
from types import SimpleNamespace

from mv2d_amd import route


def resolve(kind='S', exact=True, keep_stages=False, **options):
    opts = SimpleNamespace(**dict(route.default_options(), **options))
    return route.resolve(opts, kind, exact, 64, keep_stages=keep_stages)


def test_default_route_runs_the_fused_tail():
    assert 'fuse_qg_tail' in route.OPTIONS and route.default_options()['fuse_qg_tail'] is True
    for kind in ('S', 'T'):
        for exact in (True, False):                       # index-exact and key16
            assert resolve(kind, exact).qg_tail_fused is True


def test_keep_stages_and_the_switch_turn_it_off():
    assert resolve(keep_stages=True).qg_tail_fused is False
    assert resolve(fuse_qg_tail=False).qg_tail_fused is False
    assert resolve('T', fuse_qg_tail=False).qg_tail_fused is False


def test_environment_switch(monkeypatch):
    monkeypatch.setenv('MV2D_QG_TAIL', '0')
    assert route.default_options()['fuse_qg_tail'] is False
    monkeypatch.setenv('MV2D_QG_TAIL', '1')
    assert route.default_options()['fuse_qg_tail'] is True


def test_switch_is_launch_only():
    on, off = resolve(), resolve(fuse_qg_tail=False)
    assert 'qg_tail_fused' not in route.Storage._fields
    assert on.storage == off.storage                      # the same workspaces ...
    assert on != off                                      # ... another graph key
    assert on._replace(qg_tail_fused=False) == off        # and nothing else moves
