"""CPU-side checks of the second derivatives at scattered points (include/xnwan_hess.h, csrc/xw_tiled_paths_hvp.hip,
kernels.tiled_paths_hvp, evalpaths.start_hvp / hvp_chunk_paths / evaluate_points_hvp / evaluate_points_hess): the new header against
its ctypes table and the library, the older headers and tables as they were, the workspace query, every host-side refusal of the C
entry point, start_hvp against closed forms, the chain rule through the start value to second order against autograd's Hessian of
x -> U(x, h(x)) built from oracle.refspec, the chunk bound, and every refusal of the Python surface by its message.  No kernel is
launched."""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN, sampling, _lib  # noqa: E402
from xnode_wan_pde_solver_amd._lib import XnwanError  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NAMES = ('xw_paths_tiled_hvp_work', 'xw_paths_tiled_hvp')
FIELDS = ['xT', 'start', 'tT', 'nstep', 'Y', 'vx', 'vs', 'Yd', 'ju', 'hx', 'hs', 'N']
E_DIMS, E_ARG = -1, -2


def _header(name):
    return open(os.path.join(ROOT, 'include', name)).read()


def _declared(hdr):
    return set(re.findall(r'^\s*int\s+(xw_\w+)\s*\(', hdr, flags=re.M))


def _fields(hdr, struct):
    body = re.search(r'typedef struct \{([^}]*)\}\s*' + struct + r'\s*;', hdr).group(1)
    return [re.split(r'[\s\*]+', decl.strip())[-1] for decl in body.split(';') if decl.strip()]


def _exported():
    return subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout


def test_entry_points_are_declared_bound_and_exported():
    hdr = _header('xnwan_hess.h')
    assert '#include "xnwan.h"' in hdr
    assert _declared(hdr) == set(NAMES) == set(_lib.HESS_SIGNATURES)
    out = _exported()
    for name in NAMES:
        args = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')
        assert len(args) == len(_lib.HESS_SIGNATURES[name]), name
        assert re.search(r'\bT\s+' + name + r'\b', out), name
        assert getattr(_lib.lib, name).argtypes == _lib.HESS_SIGNATURES[name]
        assert not name.startswith('xw_tiled_')                 # (tests/test_tiled_stepper_host.py pins that set)
    assert _fields(hdr, 'XwPathsHvpJob') == [f[0] for f in _lib.XwPathsHvpJob._fields_] == FIELDS
    # what is and what is not differentiated is part of the header
    assert 'DISCRETE' in hdr and 'Time is not perturbed' in hdr and 'gates are constants' in hdr


def test_kernels_are_in_the_library_and_not_exported():
    blob = open(_lib.LIB_PATH, 'rb').read()
    assert b'kt_paths_jvp' in blob and b'kt_paths_hvp' in blob
    assert not re.findall(r'\b[A-Za-z]\s+(\S*kt_paths_(?:jvp|hvp)\S*)', _exported())


def test_the_older_headers_and_tables_are_as_they_were():
    declared = _declared(_header('xnwan.h'))
    assert len(declared) == 64 and declared == set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 33 == _lib.lib.xw_abi_version()
    assert _declared(_header('xnwan_eval.h')) == {'xw_paths_dopri5_work', 'xw_paths_dopri5_fwd'} == set(_lib.EVAL_SIGNATURES)
    assert _declared(_header('xnwan_grad.h')) == {'xw_paths_tiled_grad_work', 'xw_paths_tiled_grad'} == set(_lib.GRAD_SIGNATURES)
    assert _declared(_header('xnwan_eval_grad.h')) == {'xw_paths_dopri5_ckpt_fwd', 'xw_paths_dopri5_grad_work',
                                                       'xw_paths_dopri5_grad'} == set(_lib.EVAL_GRAD_SIGNATURES)
    assert [f[0] for f in _lib.XwPathsJob._fields_] == ['xT', 'start', 'tT', 'nstep', 'u', 'Y', 'N', 'last_only']
    assert [f[0] for f in _lib.XwPathsGradJob._fields_] == ['xT', 'start', 'tT', 'nstep', 'Y', 'gx', 'gs', 'ut', 'N'] \
        == _fields(_header('xnwan_grad.h'), 'XwPathsGradJob')
    older = (declared | set(_lib.EVAL_SIGNATURES) | set(_lib.GRAD_SIGNATURES) | set(_lib.EVAL_GRAD_SIGNATURES)
             | set(_lib.SWITCH_SIGNATURES))
    assert not set(NAMES) & older


def test_workspace_query():
    """the gradient sweep's workspace and the tangents behind it: 16 d + 8 * 16 K + 12 * 16 H + 16 doubles more per tile"""
    lib = _lib.lib
    for d, H, K, m in ((20, 20, 10, 8), (3, 65, 16, 1), (5, 96, 32, 8), (5, 256, 256, 32)):
        got = lib.xw_paths_tiled_hvp_work(d, H, K, m)
        assert got == lib.xw_paths_tiled_grad_work(d, H, K, m) + 16 * d + 8 * 16 * K + 12 * 16 * H + 16 > 0
    assert lib.xw_paths_tiled_hvp_work(20, 257, 16, 8) == -1
    assert lib.xw_paths_tiled_hvp_work(20, 20, 257, 8) == -1
    assert lib.xw_paths_tiled_hvp_work(20, 20, 10, 33) == -1
    assert lib.xw_paths_tiled_hvp_work(20, 20, 10, 0) == -1


# ---- host-side refusals, on jobs whose pointers are never dereferenced -------------------------------------------------------------
def _job(**kw):
    job = (_lib.XwPathsHvpJob * 1)()
    for k in FIELDS[:-1]:
        setattr(job[0], k, 8)                                  # (never dereferenced: every call below is refused on the host)
    job[0].N = 1
    for k, v in kw.items():
        setattr(job[0], k, v)
    return job


def _call(job, njobs=1, theta=8, method=1, L=2, d=3, H=20, K=10, m=8, work=8):
    return _lib.lib.xw_paths_tiled_hvp(job, njobs, theta, method, L, d, H, K, m, work, None)


def test_host_side_refusals_of_the_entry_point():
    assert _call(None) == E_ARG and _call(_job(), njobs=0) == E_ARG and _call(_job(), njobs=-1) == E_ARG
    assert _call(_job(), theta=None) == E_ARG and _call(_job(), work=None) == E_ARG
    for k in ('xT', 'start', 'tT', 'Y', 'vx', 'vs', 'Yd'):
        assert _call(_job(**{k: None})) == E_ARG, k
    assert _call(_job(ju=None, hx=None, hs=None)) == E_ARG
    assert _call(_job(N=0)) == E_ARG and _call(_job(N=-3)) == E_ARG
    assert _call(_job(), L=0) == E_ARG
    for method in (-1, 3, 4):
        assert _call(_job(), method=method) == E_ARG, method
    assert _call(_job(), H=257) == E_DIMS and _call(_job(), K=257) == E_DIMS and _call(_job(), m=33) == E_DIMS
    assert _call(_job(), m=0) == E_DIMS and _call(_job(), d=127) == E_DIMS


# ---- the start value's second derivative -----------------------------------------------------------------------------------------
def _first(M, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat((torch.zeros(M, 1, dtype=F64), torch.rand(M, d, generator=g, dtype=F64) * 2 - 1), 1)


def test_start_hvp_of_a_quadratic():
    first = _first(9, 4, 1)
    g = torch.Generator().manual_seed(2)
    A = torch.randn(4, 4, dtype=F64, generator=g)
    v = torch.randn(9, 4, dtype=F64, generator=g)
    b = torch.tensor([0.5, -1.0, 2.0, 0.25], dtype=F64)
    h = lambda X0: ((X0[:, 1:] @ A) * X0[:, 1:]).sum(1) + X0[:, 1:] @ b + 3 * X0[:, 0] * X0[:, 1]      # noqa: E731
    got = EP.start_hvp(h, first, v)                            # (x^T A x + b.x + 3 t x_1: the mixed (t, x) term is not in it)
    assert got.shape == (9, 4) and got.dtype == F64 and not got.requires_grad
    want = v @ (A + A.T)
    assert float((got - want).abs().max()) < 1e-14 * float(want.abs().max())
    assert not first.requires_grad and not v.requires_grad      # (the caller's tensors are left alone)
    with torch.no_grad():                                       # evaluate_points_hvp calls it under no_grad
        assert torch.equal(EP.start_hvp(h, first, v), got)


def test_start_hvp_is_exact_zeros_without_a_second_derivative():
    first = _first(5, 3, 4)
    v = torch.ones(5, 3, dtype=F64)
    zero = torch.zeros(5, 3, dtype=F64)
    for h in (lambda X0: torch.ones(X0.shape[0], dtype=F64),                                        # a constant: no grad_fn
              lambda X0: torch.full((X0.shape[0],), 2.0, dtype=F64, requires_grad=True) * 3.0,      # a graph that ignores X0
              lambda X0: torch.sin(X0[:, 0]) * 2.0,                                                 # time alone: ignores x
              lambda X0: X0[:, 1] - 2 * X0[:, 3]):                                                  # linear: a constant gradient
        got = EP.start_hvp(h, first, v)
        assert got.shape == (5, 3) and got.dtype == F64 and torch.equal(got, zero)


# ---- the chain rule through the start value, to second order -----------------------------------------------------------------------
@pytest.mark.parametrize('method', ['euler', 'midpoint', 'rk4'])
def test_chain_rule_against_the_hessian_of_the_composition(method):
    """(hx, hs, gs) -- the Hessian of the oracle's U(x, s) in (x, s) applied to (v, dh/dx . v), and dU/ds -- with start_gradient's
    dh/dx and start_hvp's d2h/dx2 . v: hx + hs dh/dx + gs d2h/dx2 v is autograd's Hessian of x -> U(x, h(x)) applied to v"""
    from oracle import refspec as R
    from test_gpu_tiled_stepper import _theta
    d, H, K, m = 3, 20, 10, 8
    theta, _ = _theta(H, K, m, d, 5)
    theta = {k: p.detach() for k, p in theta.items()}
    h = lambda X0: torch.sin(1.3 * X0[:, 1]) * X0[:, 2] + 0.5 * X0[:, 3] ** 2 + X0[:, 0]              # noqa: E731
    gen = torch.Generator().manual_seed(6)
    grid = torch.tensor([0.0, 0.2, 0.45, 0.7], dtype=F64)

    def U(x, s):                                                # refspec's arithmetic, the lift as tests/test_gpu_eval_grad.py writes it
        sv = s.view(-1, 1)
        y0 = torch.relu(torch.relu(sv @ theta['IL0_w'].T + theta['IL0_b']) @ theta['IL2_w'].T + theta['IL2_b']) @ theta['IL4_w'].T + theta['IL4_b']
        ys = R.odeint_fixed(lambda tt, y: R.field(theta, m, x.view(1, -1), tt, y), y0, grid, method)[0]
        return (ys[-1:] @ theta['FL_w'].T + theta['FL_b']).reshape(())

    for _ in range(4):
        x0 = torch.rand(d, generator=gen, dtype=F64) * 2 - 1
        v = torch.randn(d, generator=gen, dtype=F64)
        first = torch.cat((torch.zeros(1, 1, dtype=F64), x0.view(1, -1)), 1)
        dh = EP.start_gradient(h, first)[0]
        d2 = EP.start_hvp(h, first, v.view(1, -1))[0]
        x = x0.clone().requires_grad_(True)
        s = h(first).detach().clone().requires_grad_(True)
        gx, gs = torch.autograd.grad(U(x, s), [x, s], create_graph=True)
        hx, hs = torch.autograd.grad((gx * v).sum() + gs.reshape(()) * (dh * v).sum(), [x, s])
        got = hx + hs.reshape(()) * dh + gs.detach().reshape(()) * d2
        Hc = torch.autograd.functional.hessian(lambda xx: U(xx, h(torch.cat((torch.zeros(1, 1, dtype=F64), xx.view(1, -1)), 1))), x0)
        want = Hc @ v
        assert float(want.abs().max()) > 1e-8                    # (not a comparison of zeros)
        assert float((got - want).abs().max()) < 1e-12 * float(Hc.abs().max()), method


# ---- the chunk bound ----------------------------------------------------------------------------------------------------------------
def test_checkpoints_and_tangent_checkpoints_bound_the_chunk():
    assert EP.hvp_chunk_paths(65536, 9, 20) == 65536                                 # 2 * 9 * 20 * 65536 * 8 bytes: below the bound
    assert EP.hvp_chunk_paths(65536, 65, 256) == 16 * ((1 << 30) // (2 * 8 * 65 * 256 * 16)) == 4032
    assert 2 * 8 * 65 * 256 * EP.hvp_chunk_paths(65536, 65, 256) <= EP.EVAL_GRAD_CKPT_BYTES
    assert EP.hvp_chunk_paths(65536, 65, 256) * 2 <= EP.grad_chunk_paths(65536, 65, 256)   # Y and Yd: half the gradient's paths
    assert EP.hvp_chunk_paths(65536, 1 << 20, 256) == 16                             # never below one tile
    assert EP.hvp_chunk_paths(5, 9, 20) == 5


# ---- the Python surface: every refusal, on CPU tensors, before any launch -----------------------------------------------------------
SETUP = {'dim': 3, 'N_t': 4, 'T0': 0, 'T': 1, 'shape_param': 1.0}
WHO = {'hvp': r'evaluate_hvp\(\)', 'hess': r'evaluate_hess\(\)'}


def _evaluate(which, points, v=None, solver='midpoint', domain=sampling.NSphere_THourglass, n_sub=None, setup=SETUP,
              chunk=EP.EVAL_CHUNK_PATHS):
    h = lambda X0: X0[:, 1]              # noqa: E731
    tail = (n_sub, setup, domain, solver, h, torch.zeros(1, dtype=F64), KN.method_id(solver), 20, 10, 8, torch.device('cpu'))
    if which == 'hess':
        return EP.evaluate_points_hess(points, *tail, chunk=chunk)
    v = torch.zeros(points.shape[0], 3, dtype=F64) if v is None and torch.is_tensor(points) and points.dim() == 2 else v
    return EP.evaluate_points_hvp(points, v, *tail, chunk=chunk)


@pytest.mark.parametrize('which', ['hvp', 'hess'])
@pytest.mark.parametrize('solver', ['dopri5', 'explicit_adams'])
def test_the_solvers_without_a_fixed_grid_are_refused(solver, which):
    with pytest.raises(XnwanError, match=WHO[which]) as e:
        _evaluate(which, torch.zeros(2, 4, dtype=F64), solver=solver)
    assert repr(solver) in str(e.value) and 'fixed-grid' in str(e.value) and "['euler', 'midpoint', 'rk4']" in str(e.value)


@pytest.mark.parametrize('which', ['hvp', 'hess'])
def test_bad_shapes_resolutions_and_domains_are_refused(which):
    with pytest.raises(XnwanError, match=WHO[which] + r'.*\[M, 4\]'):
        _evaluate(which, torch.zeros(2, 5, dtype=F64))
    with pytest.raises(XnwanError, match=r'\[M, 4\]'):
        _evaluate(which, torch.zeros(4, dtype=F64))
    with pytest.raises(XnwanError, match=WHO[which] + '.*n_sub'):
        _evaluate(which, torch.zeros(2, 4, dtype=F64), n_sub=0)
    with pytest.raises(XnwanError, match='eval_chunk_paths'):
        _evaluate(which, torch.zeros(2, 4, dtype=F64), chunk=0)

    class Slab:
        pass
    with pytest.raises(XnwanError, match=WHO[which] + '.*Slab.*entry'):
        _evaluate(which, torch.zeros(2, 4, dtype=F64), domain=Slab)


def test_a_direction_of_another_shape_is_refused():
    pts = torch.zeros(2, 4, dtype=F64)
    for v in (torch.zeros(2, 4, dtype=F64), torch.zeros(3, dtype=F64), torch.zeros(3, 3, dtype=F64), [[0.0] * 3] * 2):
        with pytest.raises(XnwanError, match=r'evaluate_hvp\(\): v must be a tensor \[M, d\] = \[2, 3\]'):
            _evaluate('hvp', pts, v=v)


@pytest.mark.parametrize('which', ['hvp', 'hess'])
def test_points_before_their_entry_time_are_refused(which):
    with pytest.raises(XnwanError, match=WHO[which] + '.*t >= t_in') as e:
        _evaluate(which, torch.tensor([[0.5, 0.0, 0.0, 0.0], [0.1, 0.0, 0.0, 0.0]], dtype=F64), domain=sampling.Hypercube,
                  setup=dict(SETUP, T0=0.25, shape_param=[-1, 1]))
    assert '1 points' in str(e.value) and 'point 1' in str(e.value)


@pytest.mark.parametrize('which', ['hvp', 'hess'])
def test_re_entered_hourglass_points_are_refused_with_count_and_index(which):
    pts = torch.tensor([[0.25, 0.6, 0.0, 0.0], [0.75, 0.3, 0.0, 0.0], [0.75, 0.7, 0.0, 0.0], [0.0, 0.1, 0.2, 0.3],
                        [0.9, 0.0, 0.4, 0.0]], dtype=F64)
    with pytest.raises(XnwanError, match=WHO[which] + '.*entered at T0') as e:
        _evaluate(which, pts)
    assert '1 points' in str(e.value) and 'point 2' in str(e.value) and 'depends on x' in str(e.value)
    with pytest.raises(XnwanError, match='2 points'):
        _evaluate(which, torch.cat((pts, pts[2:3]), 0))


def test_no_points_give_empty_tensors():
    r = _evaluate('hvp', torch.zeros(0, 4, dtype=F64))
    assert {k: tuple(t.shape) for k, t in r.items()} == {'u': (0,), 'grad': (0, 3), 'dv': (0,), 'hvp': (0, 3)}
    q = _evaluate('hess', torch.zeros(0, 4, dtype=F64))
    assert {k: tuple(t.shape) for k, t in q.items()} == {'u': (0,), 'grad': (0, 3), 'hess': (0, 3, 3), 'lap': (0,)}
    assert all(t.dtype == F64 for t in list(r.values()) + list(q.values()))


def test_public_surface():
    from xnode_wan_pde_solver_amd import nets, solver
    assert list(inspect.signature(KN.tiled_paths_hvp).parameters) == ['jobs', 'theta', 'method', 'H', 'K', 'm', 'work']
    assert list(inspect.signature(KN.paths_hvp_work).parameters) == ['d', 'H', 'K', 'm', 'tiles', 'device']
    assert list(inspect.signature(nets.XNODE.evaluate_hvp).parameters) == ['self', 'points', 'v', 'n_sub', 'chunk']
    assert list(inspect.signature(nets.XNODE.evaluate_hess).parameters) == ['self', 'points', 'n_sub', 'chunk']
    assert list(inspect.signature(solver.NODE_WAN_solver.evaluate_hvp).parameters) == ['self', 'points', 'v', 'n_sub']
    assert list(inspect.signature(solver.NODE_WAN_solver.evaluate_hess).parameters) == ['self', 'points', 'n_sub']
    assert list(inspect.signature(solver.NODE_WAN_solver.evaluate_grad).parameters) == ['self', 'points', 'n_sub']
    for fn in (nets.XNODE.evaluate_hvp, solver.NODE_WAN_solver.evaluate_hvp, EP.evaluate_points_hvp, KN.tiled_paths_hvp):
        assert 'discrete' in fn.__doc__.lower() and 'held fixed' in fn.__doc__, fn
    from xnode_wan_pde_solver_amd.options import EngineOptions
    import dataclasses
    assert not [f.name for f in dataclasses.fields(EngineOptions) if 'hvp' in f.name or 'hess' in f.name]
