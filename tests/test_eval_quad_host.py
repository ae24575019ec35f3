"""CPU-side checks of the second-order forward jets at scattered points (include/xnwan_jet.h, csrc/xw_tiled_paths_jet.hip,
kernels.tiled_paths_jet, evalpaths.jet_chunk_paths / lap_directions / divergence_a / quad_pass / evaluate_points_quad /
evaluate_points_lap / evaluate_points_residual): the new header against its ctypes table and the library, the older headers and
tables as they were, the workspace query, every host-side refusal of the C entry point, the directions and weights of a diffusion
tensor, div a by autograd against closed forms, the chunk bound, the host chain (sort, chunks, the chain rule through the start value
to second order) with the kernel layer replaced by oracle.refspec's autograd on every path, and every refusal of the Python surface
by its message.  No kernel is launched."""
import importlib.util
import inspect
import os
import re
import subprocess
import sys
from unittest import mock

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN, sampling, _lib  # noqa: E402
from xnode_wan_pde_solver_amd._lib import XnwanError  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NAMES = ('xw_paths_tiled_jet_work', 'xw_paths_tiled_jet')
FIELDS = ['xT', 'start', 'tT', 'nstep', 'vx', 'vs', 'qs', 'u', 'ju', 'quu', 'N', 'R']
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


def _general_funcs():
    spec = importlib.util.spec_from_file_location('general_funcs', os.path.join(ROOT, 'tests', 'golden', 'general_funcs.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_points_are_declared_bound_and_exported():
    hdr = _header('xnwan_jet.h')
    assert '#include "xnwan.h"' in hdr
    assert _declared(hdr) == set(NAMES) == set(_lib.JET_SIGNATURES)
    out = _exported()
    for name in NAMES:
        args = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')
        assert len(args) == len(_lib.JET_SIGNATURES[name]), name
        assert re.search(r'\bT\s+' + name + r'\b', out), name
        assert getattr(_lib.lib, name).argtypes == _lib.JET_SIGNATURES[name]
        assert not name.startswith('xw_tiled_')                 # (tests/test_tiled_stepper_host.py pins that set)
    assert _fields(hdr, 'XwPathsJetJob') == [f[0] for f in _lib.XwPathsJetJob._fields_] == FIELDS
    # what is and what is not differentiated is part of the header
    assert 'DISCRETE' in hdr and 'Time is not perturbed' in hdr and 'gates are constants' in hdr


def test_the_kernel_is_in_the_library_and_not_exported():
    blob = open(_lib.LIB_PATH, 'rb').read()
    assert b'kt_paths_jet2' in blob
    assert not re.findall(r'\b[A-Za-z]\s+(\S*kt_paths_jet2\S*)', _exported())


def test_the_older_headers_and_tables_are_as_they_were():
    declared = _declared(_header('xnwan.h'))
    assert len(declared) == 64 and declared == set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 33 == _lib.lib.xw_abi_version()
    assert _declared(_header('xnwan_eval.h')) == {'xw_paths_dopri5_work', 'xw_paths_dopri5_fwd'} == set(_lib.EVAL_SIGNATURES)
    assert _declared(_header('xnwan_grad.h')) == {'xw_paths_tiled_grad_work', 'xw_paths_tiled_grad'} == set(_lib.GRAD_SIGNATURES)
    assert _declared(_header('xnwan_eval_grad.h')) == {'xw_paths_dopri5_ckpt_fwd', 'xw_paths_dopri5_grad_work',
                                                       'xw_paths_dopri5_grad'} == set(_lib.EVAL_GRAD_SIGNATURES)
    assert _declared(_header('xnwan_hess.h')) == {'xw_paths_tiled_hvp_work', 'xw_paths_tiled_hvp'} == set(_lib.HESS_SIGNATURES)
    assert [f[0] for f in _lib.XwPathsHvpJob._fields_] == ['xT', 'start', 'tT', 'nstep', 'Y', 'vx', 'vs', 'Yd', 'ju', 'hx', 'hs', 'N'] \
        == _fields(_header('xnwan_hess.h'), 'XwPathsHvpJob')
    older = (declared | set(_lib.EVAL_SIGNATURES) | set(_lib.GRAD_SIGNATURES) | set(_lib.EVAL_GRAD_SIGNATURES) | set(_lib.HESS_SIGNATURES)
             | set(_lib.SWITCH_SIGNATURES))
    assert not set(NAMES) & older


def test_workspace_query():
    """per block: the sweep's workspace (every layer's gates) and 16 d + 4 * 16 K + 3 * 16 H + 32 doubles behind it; -1 exactly where
    xw_tiled_ode_ok refuses"""
    lib = _lib.lib
    for d, H, K, m in ((20, 20, 10, 8), (3, 65, 16, 1), (5, 96, 32, 8), (5, 256, 256, 32)):
        got = lib.xw_paths_tiled_jet_work(d, H, K, m)
        assert got == lib.xw_paths_tiled_grad_work(d, H, K, m) + 16 * d + 4 * 16 * K + 3 * 16 * H + 32 > 0
        assert got < lib.xw_paths_tiled_hvp_work(d, H, K, m)
    for d in (1, 3, 20, 126, 127, 200):
        for H in (1, 20, 256, 257):
            for K in (1, 10, 256, 257):
                for m in (0, 1, 8, 32, 33):
                    ok = lib.xw_tiled_ode_ok(d, H, K, m)
                    assert (lib.xw_paths_tiled_jet_work(d, H, K, m) == -1) == (ok == 0), (d, H, K, m)
    assert lib.xw_paths_tiled_jet_work(20, 257, 16, 8) == -1 and lib.xw_paths_tiled_jet_work(20, 20, 257, 8) == -1
    assert lib.xw_paths_tiled_jet_work(20, 20, 10, 33) == -1 and lib.xw_paths_tiled_jet_work(20, 20, 10, 0) == -1


# ---- host-side refusals, on jobs whose pointers are never dereferenced -------------------------------------------------------------
def _job(**kw):
    job = (_lib.XwPathsJetJob * 1)()
    for k in FIELDS[:-2]:
        setattr(job[0], k, 8)                                  # (never dereferenced: every call below is refused on the host)
    job[0].N, job[0].R = 1, 1
    for k, v in kw.items():
        setattr(job[0], k, v)
    return job


def _call(job, njobs=1, theta=8, method=1, L=2, d=3, H=20, K=10, m=8, work=8):
    return _lib.lib.xw_paths_tiled_jet(job, njobs, theta, method, L, d, H, K, m, work, None)


def test_host_side_refusals_of_the_entry_point():
    assert _call(None) == E_ARG and _call(_job(), njobs=0) == E_ARG and _call(_job(), njobs=-1) == E_ARG
    assert _call(_job(), theta=None) == E_ARG and _call(_job(), work=None) == E_ARG
    for k in ('xT', 'start', 'tT', 'vx', 'vs'):
        assert _call(_job(**{k: None})) == E_ARG, k
    assert _call(_job(ju=None, quu=None)) == E_ARG
    assert _call(_job(N=0)) == E_ARG and _call(_job(N=-3)) == E_ARG
    assert _call(_job(R=0)) == E_ARG and _call(_job(R=-1)) == E_ARG and _call(_job(R=65536)) == E_ARG
    assert _call(_job(), L=0) == E_ARG
    for method in (-1, 3, 4):
        assert _call(_job(), method=method) == E_ARG, method
    assert _call(_job(), H=257) == E_DIMS and _call(_job(), K=257) == E_DIMS and _call(_job(), m=33) == E_DIMS
    assert _call(_job(), m=0) == E_DIMS and _call(_job(), d=127) == E_DIMS


# ---- directions and weights of a diffusion tensor --------------------------------------------------------------------------------------
def _points(M, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat((torch.rand(M, 1, generator=g, dtype=F64), torch.rand(M, d, generator=g, dtype=F64) * 2 - 1), 1)


def _table(fa, pts):
    M, d = pts.shape[0], pts.shape[1] - 1
    X = pts.view(M, 1, 1 + d)
    return torch.stack([torch.stack([fa(X, i, j).double().reshape(M) for j in range(d)], 1) for i in range(d)], 1)


def test_unit_directions_for_the_laplacian_and_a_diagonal_tensor():
    GF = _general_funcs()
    M, d = 7, 4
    eye = torch.eye(d, dtype=F64)
    Q, lam = EP.lap_directions(None, M, d)
    assert torch.equal(Q, eye) and torch.equal(lam, torch.ones(d, dtype=F64))
    Q, lam = EP.lap_directions(eye, M, d)
    assert torch.equal(Q, eye) and torch.equal(lam, torch.ones(d, dtype=F64))
    Q, lam = EP.lap_directions(torch.diag(torch.tensor([2.0, -1.0, 0.0, 0.5], dtype=F64)), M, d)
    assert torch.equal(Q, eye) and torch.equal(lam, torch.tensor([2.0, -1.0, 0.0, 0.5], dtype=F64))
    A = _table(GF.diag_a, _points(M, d, 3))
    Q, lam = EP.lap_directions(A, M, d)
    assert torch.equal(Q, eye) and lam.shape == (M, d) and torch.equal(lam, torch.diagonal(A, dim1=1, dim2=2))
    Q, lam = EP.lap_directions(A.float(), M, d)                   # (float32 tables are widened exactly)
    assert Q.dtype == F64 and lam.dtype == F64 and torch.equal(lam, torch.diagonal(A.float().double(), dim1=1, dim2=2))


def test_eigen_directions_rebuild_the_symmetric_part():
    GF = _general_funcs()
    M, d = 9, 4
    pts = _points(M, d, 5)
    const = _table(GF.const_a, pts[:1])[0]
    g = torch.Generator().manual_seed(6)
    lopsided = const + 0.3 * torch.triu(torch.randn(d, d, generator=g, dtype=F64), 1)      # a non-symmetric matrix
    for A, shape in ((const, (d, d)), (lopsided, (d, d)), (_table(GF.func_a, pts), (M, d, d))):
        Q, lam = EP.lap_directions(A, M, d)
        assert Q.shape == shape and lam.shape == shape[:-1] and Q.dtype == F64
        sym = 0.5 * (A + A.transpose(-1, -2))
        rebuilt = torch.einsum('...k,...ki,...kj->...ij', lam, Q, Q)
        assert float((rebuilt - sym).abs().max()) <= 1e-13 * float(sym.abs().max())
        assert float((torch.einsum('...ki,...li->...kl', Q, Q) - torch.eye(d, dtype=F64)).abs().max()) < 1e-13   # orthonormal rows
        Hs = torch.randn(M, d, d, generator=g, dtype=F64)
        Hs = Hs + Hs.transpose(1, 2)                              # ... so the weighted quadratic forms are the contraction with a Hessian
        quad = torch.einsum('...ki,mij,...kj->mk', Q, Hs, Q) if Q.dim() == 2 else torch.einsum('mki,mij,mkj->mk', Q, Hs, Q)
        want = (A * Hs).sum((-2, -1))
        assert float(((quad * lam).sum(1) - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_an_a_of_another_shape_is_refused_by_name():
    for a in (torch.zeros(3, dtype=F64), torch.zeros(3, 4, dtype=F64), torch.zeros(6, 3, 3, dtype=F64), torch.zeros(5, 3, 4, dtype=F64), 'eye'):
        with pytest.raises(XnwanError, match=r'evaluate_lap\(\): a must be None .* \[d, d\] = \[3, 3\] or \[M, d, d\] = \[5, 3, 3\]'):
            EP.lap_directions(a, 5, 3)
    with pytest.raises(XnwanError, match=r'evaluate_residual\(\): a must be'):
        EP.lap_directions(torch.zeros(2, 2), 5, 3, 'evaluate_residual()')


# ---- div a ----------------------------------------------------------------------------------------------------------------------------
def test_divergence_of_a_by_autograd():
    import configs.Ex4_1_funcs as E
    GF = _general_funcs()
    M, d = 11, 3
    pts = _points(M, d, 8)
    X = pts.view(M, 1, 1 + d)
    x1, x2 = pts[:, 1], pts[:, 2]
    want = torch.stack([x1 * (1.0 if j == 0 else 0.1 * torch.cos(x2)) + (1.0 + 0.5 * x1 ** 2) * (0.0 if j == 1 else -0.1 * torch.sin(x2))
                        for j in range(d)], 1)
    got = EP.divergence_a(GF.func_a, X, d)
    assert got.shape == (M, d) and got.dtype == F64 and not got.requires_grad and not X.requires_grad
    assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())
    with torch.no_grad():                                         # evaluate_points_residual calls it under no_grad
        assert torch.equal(EP.divergence_a(GF.func_a, X, d), got)
    got = EP.divergence_a(GF.diag_a, X, d)
    assert float((got - 0.6 * pts[:, 1:]).abs().max()) <= 1e-14
    zero = torch.zeros(M, d, dtype=F64)
    assert torch.equal(EP.divergence_a(E.func_a, X, d), zero) and torch.equal(EP.divergence_a(GF.const_a, X, d), zero)


# ---- the chunk bound ----------------------------------------------------------------------------------------------------------------
def test_the_workspace_bounds_the_chunk():
    work = _lib.lib.xw_paths_tiled_jet_work(20, 20, 10, 8)
    for chunk, R, w in ((65536, 20, work), (65536, 1, work), (65536, 100, _lib.lib.xw_paths_tiled_jet_work(100, 256, 256, 32)),
                        (1 << 20, 1, work), (65536, 3, 1 << 40)):
        per = EP.jet_chunk_paths(chunk, R, w)
        assert per % 16 == 0 and per >= 16 and per <= chunk
        tiles = per // 16
        assert tiles == 1 or tiles * R * w * 8 <= EP.EVAL_GRAD_CKPT_BYTES
        assert per == chunk or (tiles + 1) * R * w * 8 > EP.EVAL_GRAD_CKPT_BYTES     # the largest that fits
    assert EP.jet_chunk_paths(65536, 20, work) == 16 * ((1 << 30) // (8 * 20 * work)) == 12560
    assert EP.jet_chunk_paths(65536, 3, 1 << 40) == 16                               # never below one tile
    assert EP.jet_chunk_paths(5, 3, work) == 5 and EP.jet_chunk_paths(16, 3, work) == 16


# ---- the host chain, the kernel layer replaced by autograd on every path ------------------------------------------------------------
def _stub_jet(theta, m, method):
    """kernels.tiled_paths_jet's contract on the host: per path and direction ju and quu of include/xnwan_jet.h by double backward
    through oracle.refspec's arithmetic on that path alone, u its final value"""
    from oracle import refspec as R
    names = {0: 'euler', 1: 'midpoint', 2: 'rk4'}

    def U(x, s, times, mid):
        sv = s.view(-1, 1)
        y0 = torch.relu(torch.relu(sv @ theta['IL0_w'].T + theta['IL0_b']) @ theta['IL2_w'].T + theta['IL2_b']) @ theta['IL4_w'].T + theta['IL4_b']
        ys = R.odeint_fixed(lambda tt, y: R.field(theta, m, x.view(1, -1), tt, y), y0, times, names[mid])[0]
        return (ys[-1:] @ theta['FL_w'].T + theta['FL_b']).reshape(())

    calls = []

    def tiled_paths_jet(jobs, blob, mid, H, K, mm, work=None):
        with torch.enable_grad():
            for j in jobs:
                d, N = j['xT'].shape
                Rr = j['vx'].shape[0]
                calls.append((N, Rr))
                assert j['vx'].shape == (Rr, d, N) and j['vs'].shape == (Rr, N) and j['qs'].shape == (Rr, N) and j['u'].shape == (N,)
                assert all(j[k].is_contiguous() for k in ('xT', 'tT', 'vx', 'vs', 'qs', 'ju', 'quu'))
                assert work.numel() == _lib.lib.xw_paths_tiled_jet_work(d, H, K, mm) * Rr * ((N + 15) // 16)
                for i in range(N):
                    ni = int(j['nstep'][i])
                    x = j['xT'][:, i].clone().requires_grad_(True)
                    s = j['start'][i:i + 1].clone().requires_grad_(True)
                    u = U(x, s, j['tT'][:ni + 1, i], mid)
                    j['u'][i] = u.detach()
                    gx, gs = torch.autograd.grad(u, [x, s], create_graph=True, allow_unused=True)
                    gx = torch.zeros(d, dtype=F64) if gx is None else gx
                    for r in range(Rr):
                        vx, vs, qs = j['vx'][r, :, i], j['vs'][r, i], j['qs'][r, i]
                        jv = (gx * vx).sum() + gs.reshape(()) * vs
                        j['ju'][r, i] = jv.detach()
                        quu = gs.detach().reshape(()) * qs
                        if jv.requires_grad:
                            hx, hs = torch.autograd.grad(jv, [x, s], retain_graph=True, allow_unused=True)
                            quu = quu + (0.0 if hx is None else (hx * vx).sum()) + (0.0 if hs is None else hs.reshape(()) * vs)
                        j['quu'][r, i] = quu
    return tiled_paths_jet, U, calls


SETUP = {'dim': 3, 'N_t': 4, 'T0': 0, 'T': 1, 'shape_param': [-1, 1]}


@pytest.mark.parametrize('method', ['euler', 'rk4'])
def test_host_chain_against_the_hessian_of_the_composition(method):
    """evaluate_points_quad and evaluate_points_lap with the launch replaced by the stub: sort, chunks of 16, per-point directions,
    vs = dh/dx . v and qs = v . d2h/dx2 v give v^T H v and sum a_ij H_ij of autograd's Hessian of x -> U(x, h([T0, x]))"""
    from test_gpu_tiled_stepper import _theta
    GF = _general_funcs()
    d, H, K, m, M, R = 3, 20, 10, 8, 20, 2
    theta, _ = _theta(H, K, m, d, 5)
    theta = {k: p.detach() for k, p in theta.items()}
    stub, U, calls = _stub_jet(theta, m, method)
    h = lambda X0: torch.sin(1.3 * X0[:, 1]) * X0[:, 2] + 0.5 * X0[:, 3] ** 2 + X0[:, 0]              # noqa: E731
    pts = _points(M, d, 12)
    pts[0, 0], pts[1, 0] = 0.0, 1.0                                # no step; the whole interval
    V = torch.randn(M, R, d, generator=torch.Generator().manual_seed(13), dtype=F64)
    mid = KN.method_id(method)
    tail = (None, SETUP, sampling.Hypercube, method, h, torch.zeros(1, dtype=F64), mid, H, K, m, torch.device('cpu'))
    with mock.patch.object(KN, 'tiled_paths_jet', stub):
        q = EP.evaluate_points_quad(pts, V, *tail, chunk=16)
        assert calls == [(16, R), (4, R)]
        one = EP.evaluate_points_quad(pts, V, *tail)
        A = _table(GF.func_a, pts)
        lap = EP.evaluate_points_lap(pts, None, *tail)
        lap_a = EP.evaluate_points_lap(pts, A, *tail, chunk=16)
        lap_c = EP.evaluate_points_lap(pts, A[3], *tail)
    for k in q:
        assert torch.equal(q[k], one[k]), k
    n = EP.step_counts(pts[:, 0], torch.zeros(M, dtype=F64), 0, 1, 4)
    grids = EP.pack_grids(pts[:, 0], torch.zeros(M, dtype=F64), n)
    for i in range(M):
        times = grids[:int(n[i]) + 1, i]
        comp = lambda xx: U(xx, h(torch.cat((torch.zeros(1, 1, dtype=F64), xx.view(1, -1)), 1)), times, mid)   # noqa: E731
        x0 = pts[i, 1:].clone().requires_grad_(True)
        ui = comp(x0)
        gi, = torch.autograd.grad(ui, x0)
        ui = ui.detach()
        Hc = torch.autograd.functional.hessian(comp, pts[i, 1:].clone())
        scale = float(Hc.abs().max())
        assert scale > 1e-8
        assert abs(float(q['u'][i] - ui)) <= 1e-13 * abs(float(ui))
        assert float((q['dv'][i] - V[i] @ gi).abs().max()) <= 1e-12 * float(gi.abs().max())
        assert float((q['quad'][i] - torch.einsum('ri,ij,rj->r', V[i], Hc, V[i])).abs().max()) <= 1e-11 * scale, (method, i)
        assert abs(float(lap['lap'][i] - torch.trace(Hc))) <= 1e-11 * scale
        assert abs(float(lap_a['lap'][i] - (A[i] * Hc).sum())) <= 1e-11 * scale * float(A.abs().max())
        assert abs(float(lap_c['lap'][i] - (A[3] * Hc).sum())) <= 1e-11 * scale * float(A.abs().max())
    assert torch.equal(lap['u'], q['u'])


# ---- the Python surface: every refusal, on CPU tensors, before any launch -----------------------------------------------------------
HSETUP = {'dim': 3, 'N_t': 4, 'T0': 0, 'T': 1, 'shape_param': 1.0}
WHICH = ('quad', 'lap', 'residual')
WHO = {k: r'evaluate_%s\(\)' % k for k in WHICH}


def _no_launch(*a, **kw):
    raise AssertionError('a kernel wrapper was called')


def _evaluate(which, points, arg=None, solver='midpoint', domain=sampling.NSphere_THourglass, n_sub=None, setup=HSETUP,
              chunk=EP.EVAL_CHUNK_PATHS, **kw):
    import configs.Ex4_1_funcs as E
    h = lambda X0: X0[:, 1]              # noqa: E731
    tail = (n_sub, setup, domain, solver, h, torch.zeros(1, dtype=F64), KN.method_id(solver), 20, 10, 8, torch.device('cpu'))
    with mock.patch.object(KN, 'tiled_paths_jet', _no_launch), mock.patch.object(KN, 'tiled_paths_fwd', _no_launch), \
            mock.patch.object(KN, 'tiled_paths_grad', _no_launch):
        if which == 'lap':
            return EP.evaluate_points_lap(points, arg, *tail, chunk=chunk)
        if which == 'residual':
            funcs = dict(a=E.func_a, b=E.func_b, c=E.func_c, f=E.func_f) if arg is None else arg
            return EP.evaluate_points_residual(points, funcs, *tail, chunk=chunk, **kw)
        V = torch.zeros(points.shape[0], 2, 3, dtype=F64) if arg is None and torch.is_tensor(points) and points.dim() == 2 else arg
        return EP.evaluate_points_quad(points, V, *tail, chunk=chunk)


@pytest.mark.parametrize('which', WHICH)
@pytest.mark.parametrize('solver', ['dopri5', 'explicit_adams'])
def test_the_solvers_without_a_fixed_grid_are_refused(solver, which):
    with pytest.raises(XnwanError, match=WHO[which]) as e:
        _evaluate(which, torch.zeros(2, 4, dtype=F64), solver=solver)
    assert repr(solver) in str(e.value) and 'fixed-grid' in str(e.value) and "['euler', 'midpoint', 'rk4']" in str(e.value)


@pytest.mark.parametrize('which', WHICH)
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


def test_directions_and_coefficients_of_another_shape_are_refused():
    pts = torch.zeros(2, 4, dtype=F64)
    cube = dict(domain=sampling.Hypercube, setup=dict(HSETUP, shape_param=[-1, 1]))
    for V in (torch.zeros(2, 3, dtype=F64), torch.zeros(2, 2, 4, dtype=F64), torch.zeros(3, 2, 3, dtype=F64), torch.zeros(2, 0, 3, dtype=F64),
              [[[0.0] * 3]] * 2):
        with pytest.raises(XnwanError, match=r'evaluate_quad\(\): V must be a tensor \[M, R, d\] = \[2, R, 3\]'):
            _evaluate('quad', pts, V, **cube)
    for a in (torch.zeros(3, dtype=F64), torch.zeros(3, 4, dtype=F64), torch.zeros(3, 3, 3, dtype=F64), 1.0):
        with pytest.raises(XnwanError, match=r'evaluate_lap\(\): a must be None .* \[d, d\] = \[3, 3\] or \[M, d, d\] = \[2, 3, 3\]'):
            _evaluate('lap', pts, a, **cube)
    for div_a in ('closed-form', None, 3):
        with pytest.raises(XnwanError, match=r"evaluate_residual\(\): div_a must be 'autograd' or a callable"):
            _evaluate('residual', pts, div_a=div_a, **cube)


@pytest.mark.parametrize('which', WHICH)
def test_points_before_their_entry_time_are_refused(which):
    with pytest.raises(XnwanError, match=WHO[which] + '.*t >= t_in') as e:
        _evaluate(which, torch.tensor([[0.5, 0.0, 0.0, 0.0], [0.1, 0.0, 0.0, 0.0]], dtype=F64), domain=sampling.Hypercube,
                  setup=dict(HSETUP, T0=0.25, shape_param=[-1, 1]))
    assert '1 points' in str(e.value) and 'point 1' in str(e.value)


@pytest.mark.parametrize('which', WHICH)
def test_re_entered_hourglass_points_are_refused_with_count_and_index(which):
    pts = torch.tensor([[0.25, 0.6, 0.0, 0.0], [0.75, 0.3, 0.0, 0.0], [0.75, 0.7, 0.0, 0.0], [0.0, 0.1, 0.2, 0.3],
                        [0.9, 0.0, 0.4, 0.0]], dtype=F64)
    with pytest.raises(XnwanError, match=WHO[which] + '.*entered at T0') as e:
        _evaluate(which, pts)
    assert '1 points' in str(e.value) and 'point 2' in str(e.value) and 'depends on x' in str(e.value)
    with pytest.raises(XnwanError, match='2 points'):
        _evaluate(which, torch.cat((pts, pts[2:3]), 0))


def test_no_points_give_empty_tensors():
    q = _evaluate('quad', torch.zeros(0, 4, dtype=F64), torch.zeros(0, 5, 3, dtype=F64))
    assert {k: tuple(t.shape) for k, t in q.items()} == {'u': (0,), 'dv': (0, 5), 'quad': (0, 5)}
    lp = _evaluate('lap', torch.zeros(0, 4, dtype=F64))
    assert {k: tuple(t.shape) for k, t in lp.items()} == {'u': (0,), 'lap': (0,)}
    r = _evaluate('residual', torch.zeros(0, 4, dtype=F64))
    assert {k: tuple(t.shape) for k, t in r.items()} == {'u': (0,), 'ut': (0,), 'grad': (0, 3), 'diffusion': (0,), 'residual': (0,)}
    assert all(t.dtype == F64 for t in list(q.values()) + list(lp.values()) + list(r.values()))


def test_public_surface():
    from xnode_wan_pde_solver_amd import nets, solver
    assert list(inspect.signature(KN.tiled_paths_jet).parameters) == ['jobs', 'theta', 'method', 'H', 'K', 'm', 'work']
    assert list(inspect.signature(KN.paths_jet_work).parameters) == ['d', 'H', 'K', 'm', 'blocks', 'device']
    assert list(inspect.signature(nets.XNODE.evaluate_quad).parameters) == ['self', 'points', 'V', 'n_sub', 'chunk']
    assert list(inspect.signature(nets.XNODE.evaluate_lap).parameters) == ['self', 'points', 'a', 'n_sub', 'chunk']
    assert list(inspect.signature(solver.NODE_WAN_solver.evaluate_quad).parameters) == ['self', 'points', 'V', 'n_sub']
    assert list(inspect.signature(solver.NODE_WAN_solver.evaluate_lap).parameters) == ['self', 'points', 'a', 'n_sub']
    assert list(inspect.signature(solver.NODE_WAN_solver.evaluate_residual).parameters) == ['self', 'points', 'n_sub', 'div_a']
    assert inspect.signature(EP.evaluate_points_residual).parameters['div_a'].default == 'autograd'
    for fn in (nets.XNODE.evaluate_quad, solver.NODE_WAN_solver.evaluate_quad, EP.evaluate_points_quad, KN.tiled_paths_jet,
               EP.evaluate_points_lap, solver.NODE_WAN_solver.evaluate_residual, EP.evaluate_points_residual):
        assert 'discrete' in fn.__doc__.lower() and 'held fixed' in fn.__doc__, fn
    for fn in (solver.NODE_WAN_solver.evaluate_residual, EP.evaluate_points_residual):
        assert 'CONTINUOUS' in fn.__doc__ and '+ f phi' in fn.__doc__ and 'as written' in fn.__doc__, fn
    from xnode_wan_pde_solver_amd.options import EngineOptions
    import dataclasses
    assert not [f.name for f in dataclasses.fields(EngineOptions) if 'quad' in f.name or 'lap' in f.name or 'jet' in f.name or 'resid' in f.name]
