"""CPU-side checks of solver 'dopri5' in evaluate() (csrc/xw_tdopri_paths.hip, include/xnwan_eval.h, kernels.paths_dopri5_fwd,
evalpaths.evaluate_points with tol): the extension header against its ctypes table and the library, the frozen header, the
workspace query, every host-side refusal of the entry point and of evaluate_points.  No kernel is launched."""
import os
import re
import subprocess

import pytest
import torch

from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN, sampling, _lib
from xnode_wan_pde_solver_amd._lib import XnwanError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NAMES = ('xw_paths_dopri5_work', 'xw_paths_dopri5_fwd')


def _header(name):
    return open(os.path.join(ROOT, 'include', name)).read()


def test_entry_points_are_declared_bound_and_exported():
    hdr = _header('xnwan_eval.h')
    assert '#include "xnwan.h"' in hdr
    assert set(re.findall(r'^\s*int\s+(xw_\w+)\s*\(', hdr, flags=re.M)) == set(NAMES) == set(_lib.EVAL_SIGNATURES)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        args = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')
        assert len(args) == len(_lib.EVAL_SIGNATURES[name]), name
        assert re.search(r'\bT\s+' + name + r'\b', out), name
        assert getattr(_lib.lib, name).argtypes == _lib.EVAL_SIGNATURES[name]
        assert not name.startswith(('xw_tdopri5_', 'xw_tiled_'))              # (both name sets are pinned elsewhere)
    # the job struct: same field names in the same order as the ctypes mirror
    body = re.search(r'typedef struct \{([^}]*)\}\s*XwPathsDopriJob\s*;', hdr).group(1)
    fields = [re.split(r'[\s\*]+', decl.strip())[-1] for decl in body.split(';') if decl.strip()]
    assert fields == [f[0] for f in _lib.XwPathsDopriJob._fields_]
    assert fields == ['xT', 'start', 't_in', 't_end', 'u', 'status', 'n_acc', 'n_att', 'Y', 'rec', 'fin', 'N', 'cap']
    # the status codes are xnwan.h's, not redefined
    assert 'define XW_DOPRI_' not in hdr and 'XW_DOPRI_STEPS' in hdr


def test_the_frozen_header_is_as_it_was():
    hdr = _header('xnwan.h')
    declared = set(re.findall(r'^\s*int\s+(xw_\w+)\s*\(', hdr, flags=re.M))
    assert len(declared) == 64 and declared == set(_lib.SIGNATURES)
    assert not declared & set(NAMES) and not set(_lib.SIGNATURES) & set(_lib.EVAL_SIGNATURES)
    assert _lib.ABI_VERSION == 33 == _lib.lib.xw_abi_version()
    assert [f[0] for f in _lib.XwPathsJob._fields_] == ['xT', 'start', 'tT', 'nstep', 'u', 'Y', 'N', 'last_only']


def test_kernel_is_in_the_library_and_not_exported():
    assert b'kq_paths' in open(_lib.LIB_PATH, 'rb').read()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r'\b[A-Za-z]\s+(\S*kq_\S*)', out)


def test_workspace_query_is_the_tiled_dopri5_forwards():
    lib = _lib.lib
    for dims in ((20, 20, 10, 8), (3, 65, 16, 1), (5, 96, 32, 8), (5, 256, 256, 32)):
        assert lib.xw_paths_dopri5_work(*dims) == lib.xw_tdopri5_work(0, *dims) > 0
    assert lib.xw_paths_dopri5_work(20, 257, 16, 8) == -1
    assert lib.xw_paths_dopri5_work(20, 20, 10, 33) == -1


def _job(**kw):
    job = (_lib.XwPathsDopriJob * 1)()
    for k in ('xT', 'start', 't_in', 't_end', 'u', 'status', 'n_acc', 'n_att'):
        setattr(job[0], k, 8)                                  # (never dereferenced: every call below is refused on the host)
    job[0].N = 1
    for k, v in kw.items():
        setattr(job[0], k, v)
    return job


def _call(job, njobs=1, theta=8, d=3, H=20, K=10, m=8, Hn=20, rtol=1e-7, atol=1e-9, max_steps=10, max_attempts=20, work=8):
    return _lib.lib.xw_paths_dopri5_fwd(job, njobs, theta, d, H, K, m, Hn, rtol, atol, max_steps, max_attempts, work, None)


def test_host_side_refusals_of_the_entry_point():
    E_DIMS, E_ARG = -1, -2
    assert _call(None) == E_ARG and _call(_job(), njobs=0) == E_ARG
    assert _call(_job(), theta=None) == E_ARG and _call(_job(), work=None) == E_ARG
    for k in ('xT', 'start', 't_in', 't_end', 'u', 'status', 'n_acc', 'n_att'):
        assert _call(_job(**{k: None})) == E_ARG, k
    assert _call(_job(N=0)) == E_ARG and _call(_job(N=-3)) == E_ARG
    assert _call(_job(rec=8, cap=-1)) == E_ARG
    assert _call(_job(), Hn=0) == E_ARG and _call(_job(), Hn=21) == E_ARG
    assert _call(_job(), rtol=-1e-7) == E_ARG and _call(_job(), atol=-1e-9) == E_ARG and _call(_job(), rtol=float('nan')) == E_ARG
    assert _call(_job(), max_steps=0) == E_ARG and _call(_job(), max_attempts=0) == E_ARG
    assert _call(_job(), H=257, Hn=20) == E_DIMS and _call(_job(), K=257) == E_DIMS and _call(_job(), m=33) == E_DIMS
    assert _call(_job(), m=0) == E_DIMS


# ---- evaluate_points with tol ------------------------------------------------------------------------------------------------------
SETUP = {'dim': 3, 'N_t': 4, 'T0': 0, 'T': 1, 'shape_param': 1.0}
TOL = (KN.DOPRI5_RTOL, KN.DOPRI5_ATOL)


def _evaluate(points, solver='dopri5', domain=sampling.NSphere_THourglass, n_sub=None, setup=SETUP, tol=TOL):
    h = lambda X0: X0[:, 1]              # noqa: E731
    g = lambda BX: BX[..., 1]            # noqa: E731
    return EP.evaluate_points(points, n_sub, setup, domain, solver, h, g, torch.zeros(1, dtype=F64), KN.method_id(solver), 20, 10, 8,
                              torch.device('cpu'), tol=tol, Hn=20, max_steps=100)


def test_evaluate_refuses_a_step_count_with_dopri5():
    with pytest.raises(XnwanError, match='n_sub = 4') as e:
        _evaluate(torch.zeros(2, 4, dtype=F64), n_sub=4)
    assert 'dopri5' in str(e.value)


def test_evaluate_without_tol_refuses_dopri5_as_before():
    with pytest.raises(XnwanError, match='fixed-grid'):
        _evaluate(torch.zeros(2, 4, dtype=F64), tol=None)


def test_evaluate_with_tol_still_refuses_explicit_adams():
    with pytest.raises(XnwanError, match='explicit_adams') as e:
        _evaluate(torch.zeros(2, 4, dtype=F64), solver='explicit_adams')
    assert 'fixed-grid' in str(e.value)


def test_evaluate_with_tol_still_refuses_early_points():
    # the widening half, outside the inner ball: entered at |x| / r = 0.8; t = 0.7 lies before it
    pts = torch.tensor([[0.9, 0.8, 0.0, 0.0], [0.7, 0.8, 0.0, 0.0]], dtype=F64)
    with pytest.raises(XnwanError, match='t >= t_in') as e:
        _evaluate(pts)
    assert '1 points' in str(e.value) and 'point 1' in str(e.value)


def test_wrapper_surface():
    import inspect
    sig = inspect.signature(KN.paths_dopri5_fwd)
    assert list(sig.parameters) == ['jobs', 'theta', 'H', 'K', 'm', 'Hn', 'rtol', 'atol', 'max_steps', 'max_attempts']
    assert sig.parameters['rtol'].default == KN.DOPRI5_RTOL and sig.parameters['atol'].default == KN.DOPRI5_ATOL
    assert sig.parameters['max_steps'].default == KN.DOPRI5_MAX_STEPS and sig.parameters['max_attempts'].default is None
    ev = inspect.signature(EP.evaluate_points).parameters
    assert ev['tol'].default is None and ev['Hn'].default is None and 'max_steps' in ev
    with pytest.raises(XnwanError, match='eval_chunk_paths'):
        z = torch.zeros(2, dtype=F64)
        EP.paths_dopri5(torch.zeros(3, 2, dtype=F64), z, z, z, torch.zeros(1, dtype=F64), 20, 10, 8, 20, 1e-7, 1e-9, chunk=0)
