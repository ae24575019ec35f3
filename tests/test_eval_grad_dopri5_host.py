"""CPU-side checks of the gradient at scattered points with solver 'dopri5' (include/xnwan_eval_grad.h, csrc/xw_tdopri_paths_grad.hip,
the checkpointing entry of csrc/xw_tdopri_paths.hip, kernels.paths_dopri5_grad, evalpaths.dopri5_grad_chunks / evaluate_points_grad):
the new header against its ctypes table and the library, the three older headers and tables as they were, the workspace query, every
host-side refusal of the two entries, the chunk rule, and the refusals of evaluate_points_grad.  No kernel is launched."""
import inspect
import os
import re
import subprocess

import pytest
import torch

from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN, sampling, _lib
from xnode_wan_pde_solver_amd._lib import XnwanError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NAMES = ('xw_paths_dopri5_ckpt_fwd', 'xw_paths_dopri5_grad_work', 'xw_paths_dopri5_grad')
GRAD_FIELDS = ['xT', 'start', 't_in', 't_end', 'n_acc', 'rec', 'ckpt', 'Y', 'gx', 'gs', 'ut', 'N', 'cap']
E_DIMS, E_ARG = -1, -2


def _header(name):
    return open(os.path.join(ROOT, 'include', name)).read()


def _declared(hdr):
    return set(re.findall(r'^\s*int\s+(xw_\w+)\s*\(', hdr, flags=re.M))


def _fields(hdr, struct):
    body = re.search(r'typedef struct \{([^}]*)\}\s*' + struct + r'\s*;', hdr).group(1)
    return [re.split(r'[\s\*]+', decl.strip())[-1] for decl in body.split(';') if decl.strip()]


def test_entry_points_are_declared_bound_and_exported():
    hdr = _header('xnwan_eval_grad.h')
    assert '#include "xnwan_eval.h"' in hdr
    assert _declared(hdr) == set(NAMES) == set(_lib.EVAL_GRAD_SIGNATURES)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        args = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')
        assert len(args) == len(_lib.EVAL_GRAD_SIGNATURES[name]), name
        assert re.search(r'\bT\s+' + name + r'\b', out), name
        assert getattr(_lib.lib, name).argtypes == _lib.EVAL_GRAD_SIGNATURES[name]
    assert _fields(hdr, 'XwPathsDopriGradJob') == [f[0] for f in _lib.XwPathsDopriGradJob._fields_] == GRAD_FIELDS
    assert _fields(hdr, 'XwPathsDopriCkptJob') == [f[0] for f in _lib.XwPathsDopriCkptJob._fields_] == ['f', 'ckpt']
    assert _lib.XwPathsDopriCkptJob._fields_[0][1] is _lib.XwPathsDopriJob
    # what ut is, and what it is not, is part of the header
    assert 'CONTINUOUS' in hdr and 'NOT the derivative of the discrete u' in hdr


def test_kernel_is_in_the_library_and_not_exported():
    assert b'kq_paths_grad' in open(_lib.LIB_PATH, 'rb').read()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r'\b[A-Za-z]\s+(\S*kq_paths\S*)', out)


def test_the_older_headers_and_tables_are_as_they_were():
    declared = _declared(_header('xnwan.h'))
    assert len(declared) == 64 and declared == set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 33 == _lib.lib.xw_abi_version()
    assert [f[0] for f in _lib.XwPathsJob._fields_] == ['xT', 'start', 'tT', 'nstep', 'u', 'Y', 'N', 'last_only']
    assert _declared(_header('xnwan_eval.h')) == {'xw_paths_dopri5_work', 'xw_paths_dopri5_fwd'} == set(_lib.EVAL_SIGNATURES)
    assert _declared(_header('xnwan_grad.h')) == {'xw_paths_tiled_grad_work', 'xw_paths_tiled_grad'} == set(_lib.GRAD_SIGNATURES)
    assert [f[0] for f in _lib.XwPathsDopriJob._fields_] == ['xT', 'start', 't_in', 't_end', 'u', 'status', 'n_acc', 'n_att', 'Y', 'rec',
                                                             'fin', 'N', 'cap'] == _fields(_header('xnwan_eval.h'), 'XwPathsDopriJob')
    assert [f[0] for f in _lib.XwPathsGradJob._fields_] == ['xT', 'start', 'tT', 'nstep', 'Y', 'gx', 'gs', 'ut', 'N']
    older = declared | set(_lib.EVAL_SIGNATURES) | set(_lib.GRAD_SIGNATURES) | set(_lib.SWITCH_SIGNATURES)
    assert not set(NAMES) & older


def test_workspace_query_is_the_tiled_dopri5_sweeps():
    lib = _lib.lib
    for dims in ((20, 20, 10, 8), (3, 65, 16, 1), (5, 96, 32, 8), (5, 256, 256, 32)):
        assert lib.xw_paths_dopri5_grad_work(*dims) == lib.xw_tdopri5_work(1, *dims) > 0
    assert lib.xw_paths_dopri5_grad_work(20, 257, 16, 8) == -1
    assert lib.xw_paths_dopri5_grad_work(20, 20, 10, 33) == -1


# ---- host-side refusals, on jobs whose pointers are never dereferenced -------------------------------------------------------------
def _grad_job(**kw):
    job = (_lib.XwPathsDopriGradJob * 1)()
    for k in GRAD_FIELDS[:-2]:
        setattr(job[0], k, 8)
    job[0].N, job[0].cap = 1, 1
    for k, v in kw.items():
        setattr(job[0], k, v)
    return job


def _grad_call(job, njobs=1, theta=8, d=3, H=20, K=10, m=8, work=8):
    return _lib.lib.xw_paths_dopri5_grad(job, njobs, theta, d, H, K, m, work, None)


def test_host_side_refusals_of_the_sweep():
    assert _grad_call(None) == E_ARG and _grad_call(_grad_job(), njobs=0) == E_ARG and _grad_call(_grad_job(), njobs=-1) == E_ARG
    assert _grad_call(_grad_job(), theta=None) == E_ARG and _grad_call(_grad_job(), work=None) == E_ARG
    for k in ('xT', 'start', 't_in', 't_end', 'n_acc', 'rec', 'ckpt'):
        assert _grad_call(_grad_job(**{k: None})) == E_ARG, k
    assert _grad_call(_grad_job(gx=None, gs=None, ut=None)) == E_ARG
    assert _grad_call(_grad_job(Y=None)) == E_ARG                      # ut asked for without Y
    assert _grad_call(_grad_job(N=0)) == E_ARG and _grad_call(_grad_job(N=-3)) == E_ARG
    assert _grad_call(_grad_job(cap=0)) == E_ARG and _grad_call(_grad_job(cap=-1)) == E_ARG
    assert _grad_call(_grad_job(), H=257) == E_DIMS and _grad_call(_grad_job(), K=257) == E_DIMS and _grad_call(_grad_job(), m=33) == E_DIMS
    assert _grad_call(_grad_job(), m=0) == E_DIMS and _grad_call(_grad_job(), d=127) == E_DIMS


def _fwd_job(ckpt=8, **kw):
    job = (_lib.XwPathsDopriCkptJob * 1)()
    for k in ('xT', 'start', 't_in', 't_end', 'u', 'status', 'n_acc', 'n_att', 'Y', 'rec', 'fin'):
        setattr(job[0].f, k, 8)
    job[0].f.N, job[0].f.cap, job[0].ckpt = 1, 1, ckpt
    for k, v in kw.items():
        setattr(job[0].f, k, v)
    return job


def _fwd_call(job, njobs=1, theta=8, d=3, H=20, K=10, m=8, Hn=20, rtol=1e-7, atol=1e-9, max_steps=10, max_attempts=20, work=8):
    return _lib.lib.xw_paths_dopri5_ckpt_fwd(job, njobs, theta, d, H, K, m, Hn, rtol, atol, max_steps, max_attempts, work, None)


def test_host_side_refusals_of_the_checkpointing_forward():
    assert _fwd_call(None) == E_ARG and _fwd_call(_fwd_job(), njobs=0) == E_ARG
    assert _fwd_call(_fwd_job(), theta=None) == E_ARG and _fwd_call(_fwd_job(), work=None) == E_ARG
    for k in ('xT', 'start', 't_in', 't_end', 'u', 'status', 'n_acc', 'n_att'):
        assert _fwd_call(_fwd_job(**{k: None})) == E_ARG, k
    assert _fwd_call(_fwd_job(N=0)) == E_ARG
    assert _fwd_call(_fwd_job(cap=0)) == E_ARG and _fwd_call(_fwd_job(cap=-1)) == E_ARG       # a ckpt needs a slot
    assert _fwd_call(_fwd_job(ckpt=None, cap=-1)) == E_ARG                                       # ... and a rec no negative cap
    assert _fwd_call(_fwd_job(), Hn=0) == E_ARG and _fwd_call(_fwd_job(), Hn=21) == E_ARG
    assert _fwd_call(_fwd_job(), rtol=-1.0) == E_ARG and _fwd_call(_fwd_job(), atol=float('nan')) == E_ARG
    assert _fwd_call(_fwd_job(), max_steps=0) == E_ARG and _fwd_call(_fwd_job(), max_attempts=0) == E_ARG
    assert _fwd_call(_fwd_job(), H=257) == E_DIMS and _fwd_call(_fwd_job(), m=33) == E_DIMS


# ---- the chunk rule -----------------------------------------------------------------------------------------------------------------
def _covers(chunks, n, H, chunk, budget):
    assert [c[0] for c in chunks] == [0] + [c[1] for c in chunks[:-1]] and chunks[-1][1] == len(n)     # every path exactly once
    for i, (lo, hi, cap) in enumerate(chunks):
        assert 0 < hi - lo <= chunk and cap == max(1, max(n[lo:hi]))
        assert (hi - lo) % 16 == 0 or i == len(chunks) - 1 or chunk < 16
        assert 8 * cap * H * (hi - lo) <= budget or hi - lo <= 16


def test_chunks_budget_binding():
    n = [0] * 16 + [40] * 16
    budget = 8 * 40 * 256 * 16 + 8                               # one 16-path tile at cap 40, not two
    chunks = EP.dopri5_grad_chunks(n, 256, 65536, budget=budget)
    assert chunks == [(0, 16, 1), (16, 32, 40)]
    _covers(chunks, n, 256, 65536, budget)
    # a budget below one tile: one tile per chunk all the same
    assert EP.dopri5_grad_chunks(n, 256, 65536, budget=1) == [(0, 16, 1), (16, 32, 40)]
    # ... and one that holds everything: one chunk, the cap of the longest path
    assert EP.dopri5_grad_chunks(n, 256, 65536, budget=8 * 40 * 256 * 32) == [(0, 32, 40)]


def test_chunks_size_binding_and_small_clouds():
    n = sorted([3, 0, 7, 7, 1] * 11)                             # 55 paths
    for chunk in (16, 32, 40, 65536):
        chunks = EP.dopri5_grad_chunks(n, 20, chunk)
        _covers(chunks, n, 20, chunk, EP.EVAL_GRAD_CKPT_BYTES)
    assert EP.dopri5_grad_chunks(n, 20, 16) == [(0, 16, 1), (16, 32, 3), (32, 48, 7), (48, 55, 7)]
    assert EP.dopri5_grad_chunks(n, 20, 40) == [(0, 32, 3), (32, 55, 7)]       # whole tiles below the chunk size
    assert EP.dopri5_grad_chunks(n, 20, 5)[:2] == [(0, 5, 0 + 1), (5, 10, 1)]
    _covers(EP.dopri5_grad_chunks(n, 20, 5), n, 20, 5, EP.EVAL_GRAD_CKPT_BYTES)
    assert EP.dopri5_grad_chunks([4], 20, 65536) == [(0, 1, 4)]                # N = 1
    assert EP.dopri5_grad_chunks([0] * 16 + [9], 20, 65536) == [(0, 17, 9)]    # N = 17
    assert EP.dopri5_grad_chunks([0] * 16 + [9], 20, 16) == [(0, 16, 1), (16, 17, 9)]
    assert EP.dopri5_grad_chunks([0] * 17, 20, 65536) == [(0, 17, 1)]          # no step anywhere: one slot all the same
    assert EP.dopri5_grad_chunks([], 20, 65536) == []
    assert EP.dopri5_grad_chunks(torch.tensor([1, 2, 3], dtype=torch.int32), 20, 65536) == [(0, 3, 3)]
    with pytest.raises(XnwanError, match='eval_chunk_paths'):
        EP.dopri5_grad_chunks([1], 20, 0)


# ---- evaluate_points_grad: the refusals, on CPU tensors, before any launch ------------------------------------------------------------
SETUP = {'dim': 3, 'N_t': 4, 'T0': 0, 'T': 1, 'shape_param': 1.0}
TOL = (KN.DOPRI5_RTOL, KN.DOPRI5_ATOL)


def _evaluate(points, solver='dopri5', n_sub=None, **kw):
    h = lambda X0: X0[:, 1]              # noqa: E731
    return EP.evaluate_points_grad(points, n_sub, SETUP, sampling.NSphere_THourglass, solver, h, torch.zeros(1, dtype=F64),
                                   KN.method_id(solver), 20, 10, 8, torch.device('cpu'), **kw)


def test_dopri5_without_tol_gets_todays_message():
    with pytest.raises(XnwanError) as e:
        _evaluate(torch.zeros(2, 4, dtype=F64))
    assert str(e.value) == ("evaluate_grad(): solver 'dopri5' is not served -- the reverse sweep over per-path time grids runs the "
                            "fixed-grid schemes ['euler', 'midpoint', 'rk4'] only (it reverses the steps taken; no per-path step "
                            "controller or multistep history is built)")


def test_dopri5_with_tol_refuses_a_step_count():
    with pytest.raises(XnwanError, match=r"evaluate_grad\(\): n_sub = 4 with solver 'dopri5'") as e:
        _evaluate(torch.zeros(2, 4, dtype=F64), n_sub=4, tol=TOL)
    assert 'has no meaning there' in str(e.value)


@pytest.mark.parametrize('tol', [None, TOL])
def test_explicit_adams_stays_refused(tol):
    with pytest.raises(XnwanError, match='explicit_adams') as e:
        _evaluate(torch.zeros(2, 4, dtype=F64), solver='explicit_adams', tol=tol)
    assert 'fixed-grid' in str(e.value) and 'evaluate_grad' in str(e.value)


def test_with_tol_the_entry_rules_refuse_before_any_launch():
    # (the device is the CPU: reaching a kernel call would raise another error, "no GPU")
    pts = torch.tensor([[0.25, 0.6, 0.0, 0.0], [0.75, 0.3, 0.0, 0.0], [0.75, 0.7, 0.0, 0.0], [0.0, 0.1, 0.2, 0.3]], dtype=F64)
    with pytest.raises(XnwanError, match='entered at T0') as e:
        _evaluate(pts, tol=TOL)
    assert '1 points' in str(e.value) and 'point 2' in str(e.value) and 'depends on x' in str(e.value)
    with pytest.raises(XnwanError, match='eval_chunk_paths'):
        _evaluate(pts[:2], tol=TOL, chunk=0)
    r = _evaluate(torch.zeros(0, 4, dtype=F64), tol=TOL)
    assert set(r) == {'u', 'grad', 'ut'} and r['grad'].shape == (0, 3)


def test_public_surface():
    from xnode_wan_pde_solver_amd import nets, solver
    assert list(inspect.signature(KN.paths_dopri5_grad).parameters) == ['jobs', 'theta', 'H', 'K', 'm']
    p = inspect.signature(EP.evaluate_points_grad).parameters
    q = inspect.signature(EP.evaluate_points).parameters
    for k in ('tol', 'Hn', 'max_steps'):
        assert p[k].default == q[k].default, k
    assert list(inspect.signature(EP.dopri5_grad_chunks).parameters) == ['n_acc_sorted', 'H', 'chunk', 'budget']
    assert inspect.signature(EP.dopri5_grad_chunks).parameters['budget'].default == EP.EVAL_GRAD_CKPT_BYTES
    for fn in (nets.XNODE.evaluate_grad, solver.NODE_WAN_solver.evaluate_grad, EP.evaluate_points_grad, KN.paths_dopri5_grad):
        assert 'dopri5' in fn.__doc__ and 'continuous' in fn.__doc__.lower() and 'discrete' in fn.__doc__.lower(), fn
    assert 'ckpt' in KN.paths_dopri5_fwd.__doc__
