"""CPU-side checks of the tiled stepper family (csrc/xw_tiled.hip): which family serves which field, the refusal beyond its
limits, the parameter blob at the network's own widths, the option that widens its use, and that its C-ABI declarations
match the ctypes mirror.  No kernel is launched."""
import itertools
import os
import re

import pytest
import torch

from xnode_wan_pde_solver_amd import kernels as KN, nets, _lib
from xnode_wan_pde_solver_amd.options import EngineOptions
from xnode_wan_pde_solver_amd._lib import XnwanError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILED_NAMES = ('xw_tiled_ode_ok', 'xw_tiled_ode_work', 'xw_tiled_ode_bwd_slabs', 'xw_tiled_ode_fwd_multi', 'xw_tiled_ode_bwd_multi')


@pytest.mark.parametrize('H,K,m', [(20, 17, 8), (128, 64, 8), (256, 256, 32), (65, 16, 1), (96, 32, 8), (256, 128, 4)])
def test_wide_fields_take_the_tiled_family(H, K, m):
    assert KN.stepper_family(H, K, m) == 'tiled'
    assert KN.stepper_kdims(H, K, m) == (H, K)
    assert _lib.lib.xw_tiled_ode_ok(20, H, K, m) == 1


def test_served_fields_keep_their_family():
    """'mfma' / 'generic' exactly where ode_container serves today, under both policies for 'mfma'"""
    for H, K, m in itertools.product((1, 10, 20, 21, 32, 33, 64), (1, 10, 11, 12, 16), (1, 8, 10, 11, 32)):
        Hc, Kc = KN.ode_container(H, K, m)
        want = 'generic' if KN.ode_generic(Hc, Kc, m) else 'mfma'
        assert KN.stepper_family(H, K, m) == want, (H, K, m)
        assert KN.stepper_kdims(H, K, m) == (Hc, Kc)
        assert KN.stepper_family(H, K, m, 'generic') == ('tiled' if want == 'generic' else 'mfma'), (H, K, m)


@pytest.mark.parametrize('H,K,m', [(257, 16, 8), (64, 257, 8), (128, 64, 33), (128, 64, 0)])
def test_beyond_the_tiled_limits_raises_naming_them(H, K, m):
    with pytest.raises(XnwanError, match='256') as e:
        KN.stepper_family(H, K, m)
    assert 'u_hidden_dim = %d' % H in str(e.value)
    assert _lib.lib.xw_tiled_ode_ok(20, H, K, m) == 0
    assert _lib.lib.xw_tiled_ode_work(0, 20, H, K, m) == -1


def test_unknown_policy_is_refused():
    with pytest.raises(XnwanError, match='tiled_stepper'):
        KN.stepper_family(128, 64, 8, 'always')


def test_tiled_declarations_match_the_ctypes_mirror():
    hdr = open(os.path.join(ROOT, 'include', 'xnwan.h')).read()
    declared = set(re.findall(r'^\s*int\s+(xw_tiled_\w+)\s*\(', hdr, flags=re.M))
    assert declared == set(TILED_NAMES)
    for name in TILED_NAMES:
        args = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')
        assert len(args) == len(_lib.SIGNATURES[name]), name
    assert _lib.ABI_VERSION == 33 == _lib.lib.xw_abi_version()
    assert _lib.lib.xw_tiled_ode_bwd_slabs(1000) == 63 == _lib.lib.xw_ode_bwd_slabs(1000)


def test_workspace_grows_with_widths_and_depth():
    w = lambda sweep, H, K, m: _lib.lib.xw_tiled_ode_work(sweep, 20, H, K, m)  # noqa: E731
    assert 0 < w(0, 128, 64, 8) < w(1, 128, 64, 8)
    assert w(1, 128, 64, 8) < w(1, 128, 64, 9) and w(0, 128, 64, 8) < w(0, 256, 64, 8)
    assert w(0, 128, 64, 8) % 16 == 0 and w(1, 256, 256, 32) % 16 == 0


def test_a_wide_network_binds_at_its_own_widths():
    setup = {'dim': 5}
    net = nets.XNODE(128, 1, None, None, setup, 32, 8, None, solver='rk4')
    blob = net.bind(torch.device('cpu'))
    assert net.family == 'tiled' and net.kdims == (128, 32)
    assert blob.data.numel() == KN.theta_size(5, 128, 32) == sum(p.numel() for p in net.parameters())
    # plain concatenation in named_parameters() order: the state_dict is the blob
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    assert torch.equal(flat, blob.data)


def test_dopri5_at_tiled_widths_is_refused_at_bind():
    net = nets.XNODE(128, 1, None, None, {'dim': 5}, 32, 8, None, solver='dopri5')
    with pytest.raises(XnwanError, match='dopri5'):
        net.bind(torch.device('cpu'))


def test_option_reads_the_environment(monkeypatch):
    assert EngineOptions().tiled_stepper == 'beyond'
    monkeypatch.setenv('XW_TILED_STEPPER', 'generic')
    o = EngineOptions.from_env()
    assert o.tiled_stepper == 'generic' and o.non_default() == {'tiled_stepper': 'generic'}


def test_c_abi_refuses_the_adjoint_and_narrow_mode_bits():
    """xw_tiled_ode_bwd_multi returns XW_E_DIMS for mode bits 3 (adjoint) and 4 (narrow) before it reads any job or launches"""
    import ctypes
    jobs = (_lib.XwOdeBwdJob * 1)()
    jobs[0].N = 16
    dummy = ctypes.c_void_p(16)                # (never dereferenced: the refusal comes first)
    call = lambda mode: _lib.lib.xw_tiled_ode_bwd_multi(jobs, 1, dummy, dummy, 1, 4, 5, 128, 32, 8, mode, dummy, None)  # noqa: E731
    assert call(8 | 3) == -1 and call(16 | 3) == -1 and call(8 | 16 | 2) == -1
    assert call(0) == -2                       # (no output requested: XW_E_ARG)
    assert call(4 | 1) == -2                   # (x_cot_ones without parameter gradients)
    fjobs = (_lib.XwOdeFwdJob * 1)()
    assert _lib.lib.xw_tiled_ode_fwd_multi(fjobs, 1, dummy, dummy, 3, 4, 5, 128, 32, 8, None, dummy, None) == -2   # dopri5 id
    assert _lib.lib.xw_tiled_ode_fwd_multi(fjobs, 1, dummy, dummy, 1, 4, 5, 257, 32, 8, None, dummy, None) == -1   # H = 257
