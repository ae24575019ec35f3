"""CPU-side checks of the gradient at scattered points (csrc/xw_tiled_paths_grad.hip, include/xnwan_grad.h,
kernels.tiled_paths_grad, evalpaths.start_gradient / evaluate_points_grad): the extension header against its ctypes table and the
library, the frozen headers, the workspace query, every host-side refusal of the entry point, the start value's gradient against
analytic ones, and every refusal of evaluate_points_grad.  No kernel is launched."""
import math
import os
import re
import subprocess

import pytest
import torch

from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN, sampling, _lib
from xnode_wan_pde_solver_amd._lib import XnwanError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NAMES = ('xw_paths_tiled_grad_work', 'xw_paths_tiled_grad')
FIELDS = ['xT', 'start', 'tT', 'nstep', 'Y', 'gx', 'gs', 'ut', 'N']


def _header(name):
    return open(os.path.join(ROOT, 'include', name)).read()


def _declared(hdr):
    return set(re.findall(r'^\s*int\s+(xw_\w+)\s*\(', hdr, flags=re.M))


def test_entry_points_are_declared_bound_and_exported():
    hdr = _header('xnwan_grad.h')
    assert '#include "xnwan.h"' in hdr
    assert _declared(hdr) == set(NAMES) == set(_lib.GRAD_SIGNATURES)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        args = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')
        assert len(args) == len(_lib.GRAD_SIGNATURES[name]), name
        assert re.search(r'\bT\s+' + name + r'\b', out), name
        assert getattr(_lib.lib, name).argtypes == _lib.GRAD_SIGNATURES[name]
    body = re.search(r'typedef struct \{([^}]*)\}\s*XwPathsGradJob\s*;', hdr).group(1)
    fields = [re.split(r'[\s\*]+', decl.strip())[-1] for decl in body.split(';') if decl.strip()]
    assert fields == [f[0] for f in _lib.XwPathsGradJob._fields_] == FIELDS
    # what ut is, and what it is not, is part of the header
    assert 'CONTINUOUS' in hdr and 'NOT the derivative of the discrete u' in hdr


def test_kernel_is_in_the_library_and_not_exported():
    assert b'kt_paths_grad' in open(_lib.LIB_PATH, 'rb').read()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r'\b[A-Za-z]\s+(\S*kt_paths_grad\S*)', out)


def test_the_frozen_headers_are_as_they_were():
    declared = _declared(_header('xnwan.h'))
    assert len(declared) == 64 and declared == set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 33 == _lib.lib.xw_abi_version()
    assert [f[0] for f in _lib.XwPathsJob._fields_] == ['xT', 'start', 'tT', 'nstep', 'u', 'Y', 'N', 'last_only']
    assert _declared(_header('xnwan_eval.h')) == {'xw_paths_dopri5_work', 'xw_paths_dopri5_fwd'} == set(_lib.EVAL_SIGNATURES)
    assert not set(NAMES) & (declared | set(_lib.EVAL_SIGNATURES) | set(_lib.SWITCH_SIGNATURES))


def test_workspace_query_is_the_tiled_sweeps():
    lib = _lib.lib
    for dims in ((20, 20, 10, 8), (3, 65, 16, 1), (5, 96, 32, 8), (5, 256, 256, 32)):
        assert lib.xw_paths_tiled_grad_work(*dims) == lib.xw_tiled_ode_work(1, *dims) > 0
    assert lib.xw_paths_tiled_grad_work(20, 257, 16, 8) == -1
    assert lib.xw_paths_tiled_grad_work(20, 20, 10, 33) == -1


def _job(**kw):
    job = (_lib.XwPathsGradJob * 1)()
    for k in ('xT', 'start', 'tT', 'Y', 'gx', 'gs', 'ut'):
        setattr(job[0], k, 8)                                  # (never dereferenced: every call below is refused on the host)
    job[0].N = 1
    for k, v in kw.items():
        setattr(job[0], k, v)
    return job


def _call(job, njobs=1, theta=8, method=1, L=2, d=3, H=20, K=10, m=8, work=8):
    return _lib.lib.xw_paths_tiled_grad(job, njobs, theta, method, L, d, H, K, m, work, None)


def test_host_side_refusals_of_the_entry_point():
    E_DIMS, E_ARG = -1, -2
    assert _call(None) == E_ARG and _call(_job(), njobs=0) == E_ARG and _call(_job(), njobs=-1) == E_ARG
    assert _call(_job(), theta=None) == E_ARG and _call(_job(), work=None) == E_ARG
    for k in ('xT', 'start', 'tT', 'Y'):
        assert _call(_job(**{k: None})) == E_ARG, k
    assert _call(_job(gx=None, gs=None, ut=None)) == E_ARG
    assert _call(_job(N=0)) == E_ARG and _call(_job(N=-3)) == E_ARG
    assert _call(_job(), L=0) == E_ARG
    for method in (-1, 3, 4):
        assert _call(_job(), method=method) == E_ARG, method
    assert _call(_job(), H=257) == E_DIMS and _call(_job(), K=257) == E_DIMS and _call(_job(), m=33) == E_DIMS
    assert _call(_job(), m=0) == E_DIMS and _call(_job(), d=127) == E_DIMS


# ---- the start value's gradient ------------------------------------------------------------------------------------------------------
def _first(M, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat((torch.zeros(M, 1, dtype=F64), torch.rand(M, d, generator=g, dtype=F64) * 2 - 1), 1)


def test_start_gradient_of_a_quadratic():
    first = _first(9, 4, 1)
    A = torch.randn(4, 4, dtype=F64, generator=torch.Generator().manual_seed(2))
    b = torch.tensor([0.5, -1.0, 2.0, 0.25], dtype=F64)
    h = lambda X0: ((X0[:, 1:] @ A) * X0[:, 1:]).sum(1) + X0[:, 1:] @ b + 3 * X0[:, 0]      # noqa: E731  (x^T A x + b.x + 3 t)
    got = EP.start_gradient(h, first)
    assert got.shape == (9, 4) and got.dtype == F64 and not got.requires_grad
    want = first[:, 1:] @ (A + A.T) + b
    assert float((got - want).abs().max()) < 1e-14 * float(want.abs().max())
    assert not first.requires_grad                              # (the caller's tensor is left alone)
    with torch.no_grad():                                       # evaluate_points_grad calls it under no_grad
        assert torch.equal(EP.start_gradient(h, first), got)


def test_start_gradient_of_the_shipped_start_value():
    import configs.Ex4_1_funcs as P
    first = _first(7, 3, 3)
    got = EP.start_gradient(P.func_h, first)
    hp = math.pi / 2
    x1, x2 = first[:, 1], first[:, 2]
    want = torch.stack((2 * hp * torch.cos(hp * x1) * torch.cos(hp * x2), -2 * hp * torch.sin(hp * x1) * torch.sin(hp * x2),
                        torch.zeros(7, dtype=F64)), 1)
    assert float((got - want).abs().max()) < 1e-14
    for i in range(7):                                          # row by row against the Jacobian of the one-point call
        J = torch.autograd.functional.jacobian(lambda r: P.func_h(r.view(1, -1)).reshape(()), first[i])
        assert float((got[i] - J[1:]).abs().max()) < 2e-15, i  # (a few ulp of pi: the batched and the one-row sin / cos)


def test_start_gradient_of_a_constant_is_exact_zeros():
    first = _first(5, 3, 4)
    for h in (lambda X0: torch.ones(X0.shape[0], dtype=F64),                                        # no grad_fn
              lambda X0: torch.full((X0.shape[0],), 2.0, dtype=F64, requires_grad=True) * 3.0):     # a graph that does not use X0
        got = EP.start_gradient(h, first)
        assert got.shape == (5, 3) and got.dtype == F64 and torch.equal(got, torch.zeros(5, 3, dtype=F64))


# ---- evaluate_points_grad: every refusal, on CPU tensors, before any launch ----------------------------------------------------------
SETUP = {'dim': 3, 'N_t': 4, 'T0': 0, 'T': 1, 'shape_param': 1.0}


def _evaluate(points, solver='midpoint', domain=sampling.NSphere_THourglass, n_sub=None, setup=SETUP, chunk=EP.EVAL_CHUNK_PATHS):
    h = lambda X0: X0[:, 1]              # noqa: E731
    return EP.evaluate_points_grad(points, n_sub, setup, domain, solver, h, torch.zeros(1, dtype=F64), KN.method_id(solver), 20, 10, 8,
                                   torch.device('cpu'), chunk=chunk)


@pytest.mark.parametrize('solver', ['dopri5', 'explicit_adams'])
def test_the_solvers_without_a_fixed_grid_are_refused(solver):
    with pytest.raises(XnwanError, match=solver) as e:
        _evaluate(torch.zeros(2, 4, dtype=F64), solver=solver)
    assert 'fixed-grid' in str(e.value) and 'evaluate_grad' in str(e.value)


def test_bad_shapes_resolutions_and_domains_are_refused():
    with pytest.raises(XnwanError, match=r'\[M, 4\]'):
        _evaluate(torch.zeros(2, 5, dtype=F64))
    with pytest.raises(XnwanError, match=r'\[M, 4\]'):
        _evaluate(torch.zeros(4, dtype=F64))
    with pytest.raises(XnwanError, match='n_sub'):
        _evaluate(torch.zeros(2, 4, dtype=F64), n_sub=0)
    with pytest.raises(XnwanError, match='eval_chunk_paths'):
        _evaluate(torch.zeros(2, 4, dtype=F64), chunk=0)

    class Slab:
        pass
    with pytest.raises(XnwanError, match='Slab.*entry'):
        _evaluate(torch.zeros(2, 4, dtype=F64), domain=Slab)


def test_points_before_their_entry_time_are_refused():
    with pytest.raises(XnwanError, match='t >= t_in') as e:
        _evaluate(torch.tensor([[0.5, 0.0, 0.0, 0.0], [0.1, 0.0, 0.0, 0.0]], dtype=F64), domain=sampling.Hypercube,
                  setup=dict(SETUP, T0=0.25, shape_param=[-1, 1]))
    assert '1 points' in str(e.value) and 'point 1' in str(e.value)


def test_re_entered_hourglass_points_are_refused_with_count_and_index():
    # four points entered at T0 (narrowing half; widening half inside the inner ball) and, at index 2, one that left the inner ball
    # and came back through the moving boundary at |x| / r = 0.7
    pts = torch.tensor([[0.25, 0.6, 0.0, 0.0], [0.75, 0.3, 0.0, 0.0], [0.75, 0.7, 0.0, 0.0], [0.0, 0.1, 0.2, 0.3],
                        [0.9, 0.0, 0.4, 0.0]], dtype=F64)
    _, at_T0 = sampling.NSphere_THourglass.entry(pts, 1.0, 0, 1)
    assert at_T0.tolist() == [True, True, False, True, True]
    with pytest.raises(XnwanError, match='entered at T0') as e:
        _evaluate(pts)
    assert '1 points' in str(e.value) and 'point 2' in str(e.value) and 'depends on x' in str(e.value)
    with pytest.raises(XnwanError, match='2 points'):
        _evaluate(torch.cat((pts, pts[2:3]), 0))


def test_no_points_give_empty_tensors():
    r = _evaluate(torch.zeros(0, 4, dtype=F64))
    assert set(r) == {'u', 'grad', 'ut'}
    assert r['u'].shape == (0,) and r['grad'].shape == (0, 3) and r['ut'].shape == (0,)
    assert all(v.dtype == F64 for v in r.values())


def test_the_checkpoints_bound_the_chunk():
    assert EP.EVAL_GRAD_CKPT_BYTES == 1 << 30
    assert EP.grad_chunk_paths(65536, 9, 20) == 65536                                # 9 * 20 * 65536 * 8 bytes: below the bound
    assert EP.grad_chunk_paths(65536, 65, 256) == 16 * ((1 << 30) // (8 * 65 * 256 * 16)) == 8064
    assert EP.grad_chunk_paths(65536, 1 << 20, 256) == 16                            # never below one tile
    assert EP.grad_chunk_paths(5, 9, 20) == 5


def test_public_surface_exists():
    import inspect
    from xnode_wan_pde_solver_amd import nets, solver
    assert list(inspect.signature(nets.XNODE.evaluate_grad).parameters) == ['self', 'points', 'n_sub', 'chunk']
    assert list(inspect.signature(solver.NODE_WAN_solver.evaluate_grad).parameters) == ['self', 'points', 'n_sub']
    assert list(inspect.signature(KN.tiled_paths_grad).parameters) == ['jobs', 'theta', 'method', 'H', 'K', 'm']
    for fn in (nets.XNODE.evaluate_grad, solver.NODE_WAN_solver.evaluate_grad, EP.evaluate_points_grad, KN.tiled_paths_grad):
        assert 'continuous' in fn.__doc__.lower() and 'discrete' in fn.__doc__.lower(), fn
    # evaluate() is as it was: it still says so
    assert 'No gradients' in nets.XNODE.evaluate.__doc__
