"""Host side of the cached x-projection table (EngineOptions.xproj_cached): option defaults and environment, what plan() reports,
the validity key against a stub group, and the C ABI (same symbols, same version, XwGroup grown by one int at its end).  No GPU."""
import ctypes
import os
import re
import types

from xnode_wan_pde_solver_amd import _lib
from xnode_wan_pde_solver_amd.engine import Engine
from xnode_wan_pde_solver_amd.options import EngineOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_defaults_and_environment(monkeypatch):
    o = EngineOptions()
    assert o.xproj_cached is True and o.xproj_min_d == 45 and 1 <= o.xproj_cached_min_d <= o.xproj_min_d
    for k in ('XW_XPROJ_CACHED', 'XW_XPROJ_CACHED_MIN_D', 'XW_XPROJ_MIN_D'):
        monkeypatch.delenv(k, raising=False)
    e = EngineOptions.from_env()
    assert (e.xproj_cached, e.xproj_cached_min_d, e.xproj_min_d) == (o.xproj_cached, o.xproj_cached_min_d, o.xproj_min_d)
    monkeypatch.setenv('XW_XPROJ_CACHED', '0')
    monkeypatch.setenv('XW_XPROJ_CACHED_MIN_D', '7')
    e = EngineOptions.from_env()
    assert e.xproj_cached is False and e.xproj_cached_min_d == 7 and e.xproj_min_d == 45
    assert e.non_default() == {'xproj_cached': False, 'xproj_cached_min_d': 7}
    monkeypatch.setenv('XW_XPROJ_CACHED', '1')
    monkeypatch.setenv('XW_XPROJ_MIN_D', '1')
    e = EngineOptions.from_env()
    assert e.xproj_cached is True and e.xproj_min_d == 1


class _Param:
    def __init__(self):
        self._version = 0


class _StubEngine:
    """the bookkeeping methods of Engine over plain attributes (nothing here touches a device)"""
    _v_key, _v_fresh, _xproj_held, _xproj_tail, _xproj_state, invalidate_test_net, xproj_plan, disc = (
        Engine._v_key, Engine._v_fresh, Engine._xproj_held, Engine._xproj_tail, Engine._xproj_state, Engine.invalidate_test_net,
        Engine.xproj_plan, Engine._disc_bookkeeping)     # (disc: the bookkeeping discriminator_step itself runs)

    def __init__(self, cached=True, reuse=False):
        self.xproj_cached, self.reuse_test_net, self.accum_v, self._phi_version = cached, reuse, None, 0
        self.phi = types.SimpleNamespace(params=[_Param(), _Param()])

    def formed(self, G):
        """what _form_xproj / the launch behind Adam record"""
        G.xproj_key = self._v_key(G)


def _group(table=True, tpp=None, N=33):
    return types.SimpleNamespace(N=N, tpp=tpp, _lazy={'xproj': (0, (64, N))} if table else {}, sample_version=0, vact=None)


def test_key_match_and_every_way_it_breaks():
    E, G = _StubEngine(), _group()
    assert E._v_fresh(G) == '' and not G.xproj_cur                    # first use of a group: formed at the head ...
    assert E._v_fresh(G) == '_xc' and G.xproj_cur                     # ... and current from then on
    E.formed(G)
    assert E._v_fresh(G) == '_xc'
    assert E.disc(G) == '_xc' and E._v_fresh(G) == '_xc'              # the engine's own update of phi: formed again behind it
    E.invalidate_test_net()                                           # phi bump from outside
    assert E._v_fresh(G) == '' and not G.xproj_cur
    assert E._v_fresh(G) == '_xc'
    E.phi.params[1]._version += 1                                     # torch-side in-place write
    assert E._v_fresh(G) == '' and E._v_fresh(G) == '_xc'
    G.sample_version += 1                                             # resample without the load-time launch
    assert E._v_fresh(G) == '' and E._v_fresh(G) == '_xc'
    G.sample_version += 1
    E.formed(G)                                                       # resample with it
    assert E._v_fresh(G) == '_xc'


def test_key_of_the_groups_that_keep_no_table():
    for E, G in ((_StubEngine(cached=False), _group()), (_StubEngine(), _group(table=False)), (_StubEngine(), _group(tpp=object())),
                 (_StubEngine(), _group(N=0))):
        E.formed(G)
        assert E._v_fresh(G) == '' and not G.xproj_cur and not E._xproj_tail(G)
        assert E.disc(G) == '' and not G.xproj_cur
    # a carried gradient (several groups per sub-iteration): phi moves again before this group's next sub-step -- no launch
    # behind Adam, and the key does not claim one
    E, G = _StubEngine(), _group()
    E.formed(G)
    E.accum_v = object()
    assert E.disc(G) == '_xc' and not E._xproj_tail(G)
    assert E._v_fresh(G) == ''
    # reuse_test_net: a sub-step that skips the test network decides nothing about the table
    E, G = _StubEngine(reuse=True), _group()
    assert E._v_fresh(G) == '' and E._v_fresh(G) == '_vcached' and not G.xproj_cur


def test_plan_reports_the_switch():
    mk = lambda **kw: types.SimpleNamespace(**dict(dict(xproj_min_d=45, xproj_table_min_d=20, xproj_cached=True, d=20, testnet_tiled=False), **kw))  # noqa: E731
    assert 'cached' in Engine.xproj_plan(mk()) and 'from d = 20' in Engine.xproj_plan(mk())
    assert Engine.xproj_plan(mk(d=5)).startswith('per point')
    assert 'head of every' in Engine.xproj_plan(mk(xproj_cached=False, xproj_table_min_d=45, d=50))
    assert 'tiled' in Engine.xproj_plan(mk(xproj_min_d=1 << 30, testnet_tiled=True, xproj_cached=False))


def test_abi_same_symbols_same_version_one_int_at_the_end():
    hdr = open(os.path.join(ROOT, 'include', 'xnwan.h')).read()
    assert _lib.ABI_VERSION == 33 and _lib.lib.xw_abi_version() == 33
    declared = set(re.findall(r'^\s*int\s+(xw_\w+)\s*\(', hdr, flags=re.M))
    assert declared == set(_lib.SIGNATURES) and len(declared) == 64
    assert {'xw_disc_xproj', 'xw_disc_fwd_xproj', 'xw_substep_gen', 'xw_substep_disc'} <= declared
    f = _lib.XwGroup._fields_
    assert f[-1] == ('xproj_current', ctypes.c_int) and f[-2][0] == 'xproj'
    assert [n for n, _ in f].count('xproj_current') == 1
    # ... at the end: every field of before keeps its offset
    assert _lib.XwGroup.xproj_current.offset == _lib.XwGroup.xproj.offset + ctypes.sizeof(ctypes.c_void_p)
    body = re.search(r'typedef struct \{([^}]*)\}\s*XwGroup\s*;', hdr).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    assert [d.strip() for d in body.split(';') if d.strip()][-1] == 'int xproj_current'
