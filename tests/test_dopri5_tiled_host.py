"""CPU-side checks of solver 'dopri5' on the tiled stepper family (csrc/xw_tdopri.hip, selected by dopri5_stepper = 'tiled'): the
option, its C-ABI declarations against the ctypes mirror and the exported symbols, the work-size functions, the refusals of the
entry points before they read a job, and where a wide dopri5 network binds.  No kernel is launched."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from xnode_wan_pde_solver_amd import kernels as KN, nets, _lib
from xnode_wan_pde_solver_amd.options import EngineOptions
from xnode_wan_pde_solver_amd._lib import XnwanError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDOPRI_NAMES = ('xw_tdopri5_work', 'xw_tdopri5_part_size', 'xw_tdopri5_init', 'xw_tdopri5_attempts', 'xw_tdopri5_sweep')


def test_option_default_environment_and_unknown_values(monkeypatch):
    assert EngineOptions().dopri5_stepper == 'vector'
    monkeypatch.delenv('XW_DOPRI5_STEPPER', raising=False)
    o = EngineOptions.from_env()
    assert o.dopri5_stepper == 'vector' and 'dopri5_stepper' not in o.non_default()
    monkeypatch.setenv('XW_DOPRI5_STEPPER', '')
    assert EngineOptions.from_env().dopri5_stepper == 'vector'
    monkeypatch.setenv('XW_DOPRI5_STEPPER', 'tiled')
    o = EngineOptions.from_env()
    assert o.dopri5_stepper == 'tiled' and o.non_default()['dopri5_stepper'] == 'tiled'
    assert KN.DOPRI5_STEPPERS == ('vector', 'tiled')
    assert KN.dopri5_stepper('vector') == 'vector' and KN.dopri5_stepper('tiled') == 'tiled'
    with pytest.raises(XnwanError) as e:
        KN.dopri5_stepper('mfma')
    assert "'vector'" in str(e.value) and "'tiled'" in str(e.value)


def test_an_unknown_stepper_is_refused_where_it_is_used():
    net = nets.XNODE(128, 1, None, None, {'dim': 5}, 32, 8, None, solver='dopri5')
    net.dopri5_stepper = 'matrix'
    with pytest.raises(XnwanError, match="'vector'.*'tiled'"):
        net.bind(torch.device('cpu'))
    from xnode_wan_pde_solver_amd.engine import Engine
    cfg = {'solver': 'dopri5', 'adjoint': False, 'alpha': 1.0}
    with pytest.raises(XnwanError, match="'vector'.*'tiled'"):
        Engine(cfg, {'dim': 3}, None, None, None, torch.device('cpu'), options=EngineOptions(dopri5_stepper='matrix'))
    with pytest.raises(XnwanError, match="'vector'.*'tiled'"):
        KN.Dopri5Record(16, 20, 4, torch.device('cpu'), 'matrix')


def test_declarations_match_the_ctypes_mirror_and_the_exports():
    hdr = open(os.path.join(ROOT, 'include', 'xnwan.h')).read()
    declared = set(re.findall(r'^\s*int\s+(xw_tdopri5_\w+)\s*\(', hdr, flags=re.M))
    assert declared == set(TDOPRI_NAMES)
    for name in TDOPRI_NAMES:
        args = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')
        assert len(args) == len(_lib.SIGNATURES[name]), name
    # the same job structs plus the workspace pointer: one argument more than the vector implementation's launches
    for name in ('init', 'attempts', 'sweep'):
        assert len(_lib.SIGNATURES['xw_tdopri5_' + name]) == len(_lib.SIGNATURES['xw_dopri5_' + name]) + 1
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(TDOPRI_NAMES) <= set(re.findall(r'\bT\s+(xw_\w+)', out))
    assert not re.findall(r'\bT\s+(\S*kq_\S*)', out)                       # (the kernels stay in the anonymous namespace)
    assert _lib.ABI_VERSION == 33 == _lib.lib.xw_abi_version()


def test_work_sizes():
    w = lambda sweep, H, K, m, d=20: _lib.lib.xw_tdopri5_work(sweep, d, H, K, m)  # noqa: E731
    for H, K, m in ((20, 10, 8), (128, 64, 8), (65, 16, 1), (256, 256, 32)):
        assert 0 < w(0, H, K, m) < w(1, H, K, m)
        assert w(0, H, K, m) % 16 == 0 and w(1, H, K, m) % 16 == 0
        # the forward holds k_0 .. k_6, a stage input and temporaries as H-vectors of 16 paths; the sweep also their cotangents
        assert w(0, H, K, m) >= 16 * H * 9 and w(1, H, K, m) >= 16 * H * 18
    assert w(0, 128, 64, 8) < w(0, 256, 64, 8) and w(1, 128, 64, 8) < w(1, 256, 64, 8)
    assert w(0, 128, 64, 8) < w(0, 128, 128, 8) and w(1, 128, 64, 8) < w(1, 128, 128, 8)
    assert w(1, 128, 64, 8) < w(1, 128, 64, 9)
    assert w(0, 128, 64, 8, d=3) < w(0, 128, 64, 8, d=20)
    for sweep in (0, 1):
        assert w(sweep, 257, 64, 8) == -1 and w(sweep, 128, 257, 8) == -1 and w(sweep, 128, 64, 33) == -1 and w(sweep, 128, 64, 0) == -1
    p = _lib.lib.xw_tdopri5_part_size
    assert (p(1), p(16), p(17), p(37), p(4096)) == (2, 2, 4, 6, 512)         # two doubles per 16-path tile
    assert p(0) == -2
    assert p(4096) == 4 * _lib.lib.xw_dopri5_work_size(4096)


def test_c_abi_refusals_come_before_any_job_is_read():
    """XW_E_DIMS (-1) beyond 256 / 256 / 32 and for mode bits 3 and 4, XW_E_ARG (-2) for L < 1, njobs outside 1..8, no requested
    output and x_cot_ones without both outputs -- with job arrays and pointers that are never dereferenced"""
    lib = _lib.lib
    dummy = ctypes.c_void_p(16)
    fjobs = (_lib.XwDopriJob * 9)()
    sjobs = (_lib.XwDopriSweepJob * 9)()

    def init(njobs=1, L=4, H=128, K=32, m=8):
        return lib.xw_tdopri5_init(fjobs, njobs, dummy, dummy, L, 5, H, K, m, H, 1e-7, 1e-9, dummy, None)

    def attempts(njobs=1, L=4, H=128, K=32, m=8):
        return lib.xw_tdopri5_attempts(fjobs, njobs, dummy, dummy, L, 5, H, K, m, H, 1e-7, 1e-9, 100, 1, dummy, None)

    def sweep(mode=3, njobs=1, L=4, H=128, K=32, m=8):
        return lib.xw_tdopri5_sweep(sjobs, njobs, dummy, dummy, L, 5, H, K, m, mode, dummy, None)

    for call in (init, attempts, sweep):
        assert call(H=257) == -1 and call(K=257) == -1 and call(m=33) == -1 and call(m=0) == -1
        assert call(L=0) == -2
        assert call(njobs=0) == -2 and call(njobs=9) == -2
        # (a zeroed job -- null pointers, N = 0 -- is XW_E_ARG as well, once the scalars pass)
        assert call() == -2
    assert sweep(mode=8 | 3) == -1 and sweep(mode=16 | 3) == -1 and sweep(mode=8 | 16 | 2) == -1
    assert sweep(mode=0) == -2                                              # no output requested
    assert sweep(mode=4 | 1) == -2 and sweep(mode=4 | 2) == -2             # x_cot_ones without both outputs
    # the scalar refusals do not depend on what the jobs hold: the job array may be a pointer that cannot be read
    bad = ctypes.cast(ctypes.c_void_p(16), ctypes.POINTER(_lib.XwDopriJob))
    assert lib.xw_tdopri5_init(bad, 1, dummy, dummy, 4, 5, 257, 32, 8, 257, 1e-7, 1e-9, dummy, None) == -1
    assert lib.xw_tdopri5_attempts(bad, 9, dummy, dummy, 4, 5, 128, 32, 8, 128, 1e-7, 1e-9, 100, 1, dummy, None) == -2
    sbad = ctypes.cast(ctypes.c_void_p(16), ctypes.POINTER(_lib.XwDopriSweepJob))
    assert lib.xw_tdopri5_sweep(sbad, 1, dummy, dummy, 4, 5, 128, 32, 8, 8 | 3, dummy, None) == -1
    assert lib.xw_tdopri5_sweep(sbad, 1, dummy, dummy, 0, 5, 128, 32, 8, 3, dummy, None) == -2


def test_a_wide_dopri5_network_binds_with_the_tiled_stepper():
    net = nets.XNODE(128, 1, None, None, {'dim': 5}, 32, 8, None, solver='dopri5')
    assert net.dopri5_stepper == 'vector'
    with pytest.raises(XnwanError, match='dopri5_stepper'):
        net.bind(torch.device('cpu'))
    net.dopri5_stepper = 'tiled'
    blob = net.bind(torch.device('cpu'))
    assert net.family == 'tiled' and net.kdims == (128, 32)
    assert blob.data.numel() == KN.theta_size(5, 128, 32) == sum(p.numel() for p in net.parameters())
    # at the fused containers' widths the option changes nothing about where the network binds
    small = nets.XNODE(12, 1, None, None, {'dim': 5}, 6, 8, None, solver='dopri5')
    small.dopri5_stepper = 'tiled'
    small.bind(torch.device('cpu'))
    assert small.family == 'mfma' and small.kdims == KN.ode_container(12, 6, 8) == (20, 10)
    # the family functions and the fixed-grid ids are what they were
    assert KN.method_id('dopri5') == KN.DOPRI5 == 3 and 'dopri5' not in KN.METHODS
    assert KN.stepper_family(128, 32, 8, method=KN.DOPRI5) == 'tiled' and KN.stepper_family(20, 10, 8, method=KN.DOPRI5) == 'mfma'


def test_two_ranks_and_the_adjoint_stay_refused_under_the_tiled_stepper():
    from xnode_wan_pde_solver_amd.engine import Engine
    cfg = {'solver': 'dopri5', 'adjoint': False, 'alpha': 1.0}

    class TwoRanks:
        size = 2
    with pytest.raises(XnwanError, match="'dopri5' runs on one GPU"):
        Engine(cfg, {'dim': 3}, None, None, None, torch.device('cpu'), world=TwoRanks(), options=EngineOptions(dopri5_stepper='tiled'))
    with pytest.raises(XnwanError, match="'dopri5' with adjoint=True"):
        nets.XNODE(128, 1, None, None, {'dim': 3}, 32, 8, None, solver='dopri5', adjoint=True)


def test_the_rate_tool_takes_the_stepper_and_the_shape():
    r = subprocess.run([os.sys.executable, os.path.join(ROOT, 'tools', 'dopri5_rate.py'), '--help'], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', '')))
    assert r.returncode == 0, r.stderr[-2000:]
    assert '--stepper' in r.stdout and '--shape' in r.stdout and 'both' in r.stdout
