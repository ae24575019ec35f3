"""CPU-side checks of the parameter gradients of u, du/dx and ut at scattered points (include/xnwan_grad_vjp.h,
csrc/xw_tiled_paths_gvjp.hip, kernels.tiled_paths_gvjp / paths_gvjp_work, evalpaths.gvjp_chunk_paths / evaluate_points_grad_vjp,
XNODE.evaluate_grad_vjp / evaluate_grad_fn, NODE_WAN_solver.evaluate_grad_vjp): the new header against its ctypes table and the
library, the older headers and tables as they were, the workspace query, every host-side refusal of the C entry point, the chunk
bound, every refusal of the Python surface by its message before any launch, the empty cloud, the public signatures -- and the
reference's own floor: oracle.refspec's reverse-over-reverse value of the gradient against forward-over-reverse
(tests/grad_vjp_oracle.py).  No kernel is launched."""
import inspect
import os
import re
import subprocess
import sys
from unittest import mock

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_vjp_oracle as O  # noqa: E402
from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN, nets, sampling, solver, _lib  # noqa: E402
from xnode_wan_pde_solver_amd._lib import XnwanError  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NAMES = ('xw_paths_tiled_gvjp_work', 'xw_paths_tiled_gvjp')
FIELDS = ['xT', 'start', 'tT', 'nstep', 'Y', 'Yd', 'vx', 'vs', 'wu', 'wt', 'gslab', 'N']
E_DIMS, E_ARG = -1, -2
NETS = ((3, 20, 10, 8), (20, 65, 16, 1), (5, 96, 32, 8))          # (d, H, K, m): tests/test_gpu_eval_paths.py's
FLOOR = 1e-12                                                      # two orders inside the device's bound, 1e-10 of a block's scale


def _header(name):
    return open(os.path.join(ROOT, 'include', name)).read()


def _declared(hdr):
    return set(re.findall(r'^\s*int\s+(xw_\w+)\s*\(', hdr, flags=re.M))


def _fields(hdr, struct):
    body = re.search(r'typedef struct \{([^}]*)\}\s*' + struct + r'\s*;', hdr).group(1)
    return [re.split(r'[\s\*]+', decl.strip())[-1] for decl in body.split(';') if decl.strip()]


def _exported():
    return subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    hdr = _header('xnwan_grad_vjp.h')
    assert '#include "xnwan_hess.h"' in hdr and '#include "xnwan_vjp.h"' in hdr
    assert _declared(hdr) == set(NAMES) == set(_lib.GVJP_SIGNATURES)
    out = _exported()
    for name in NAMES:
        args = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')
        assert len(args) == len(_lib.GVJP_SIGNATURES[name]), name
        assert re.search(r'\bT\s+' + name + r'\b', out), name
        assert getattr(_lib.lib, name).argtypes == _lib.GVJP_SIGNATURES[name]
        assert name.startswith('xw_paths_')
    assert _fields(hdr, 'XwPathsGvjpJob') == [f[0] for f in _lib.XwPathsGvjpJob._fields_] == FIELDS
    # what is differentiated and held fixed, who writes Yd, and the slab format, are part of the header
    assert 'DISCRETE' in hdr and 'held fixed' in hdr and 'constants of theta' in hdr and 'ReLU gates constants' in hdr
    assert 'CONTINUOUS' in hdr and 'Yd is READ here' in hdr and 'with ju alone' in hdr
    assert 'xw_slab_sum' in hdr and 'zeroes it on the stream' in hdr


def test_the_kernel_is_in_the_library_and_not_exported():
    blob = open(_lib.LIB_PATH, 'rb').read()
    assert b'kt_paths_gvjp' in blob
    assert not re.findall(r'\b[A-Za-z]\s+(\S*kt_paths_gvjp\S*)', _exported())


def test_the_older_headers_and_tables_are_as_they_were():
    declared = _declared(_header('xnwan.h'))
    assert len(declared) == 64 and declared == set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 33 == _lib.lib.xw_abi_version()
    assert _declared(_header('xnwan_hess.h')) == {'xw_paths_tiled_hvp_work', 'xw_paths_tiled_hvp'} == set(_lib.HESS_SIGNATURES)
    assert _declared(_header('xnwan_vjp.h')) == {'xw_paths_tiled_vjp_work', 'xw_paths_tiled_vjp'} == set(_lib.VJP_SIGNATURES)
    assert _declared(_header('xnwan_grad.h')) == {'xw_paths_tiled_grad_work', 'xw_paths_tiled_grad'} == set(_lib.GRAD_SIGNATURES)
    assert _declared(_header('xnwan_jet.h')) == {'xw_paths_tiled_jet_work', 'xw_paths_tiled_jet'} == set(_lib.JET_SIGNATURES)
    assert [f[0] for f in _lib.XwPathsVjpJob._fields_] == ['xT', 'start', 'tT', 'nstep', 'Y', 'w', 'gslab', 'gx', 'gs', 'N'] \
        == _fields(_header('xnwan_vjp.h'), 'XwPathsVjpJob')
    assert [f[0] for f in _lib.XwPathsHvpJob._fields_] == ['xT', 'start', 'tT', 'nstep', 'Y', 'vx', 'vs', 'Yd', 'ju', 'hx', 'hs', 'N'] \
        == _fields(_header('xnwan_hess.h'), 'XwPathsHvpJob')
    older = (declared | set(_lib.EVAL_SIGNATURES) | set(_lib.GRAD_SIGNATURES) | set(_lib.EVAL_GRAD_SIGNATURES) | set(_lib.HESS_SIGNATURES)
             | set(_lib.JET_SIGNATURES) | set(_lib.VJP_SIGNATURES) | set(_lib.SWITCH_SIGNATURES))
    assert not set(NAMES) & older


def test_workspace_query():
    """per tile: the Hessian-vector sweep's workspace, then the 16 stage times, the 16 weights on ut and a tangent per layer of the
    field; -1 exactly where xw_tiled_ode_ok refuses"""
    lib = _lib.lib
    for d, H, K, m in ((20, 20, 10, 8), (3, 65, 16, 1), (5, 96, 32, 8), (5, 256, 256, 32)):
        got = lib.xw_paths_tiled_gvjp_work(d, H, K, m)
        assert got >= lib.xw_paths_tiled_hvp_work(d, H, K, m) + 16 > 16
        assert got == lib.xw_paths_tiled_hvp_work(d, H, K, m) + 32 + 16 * K * m
    for d in (1, 3, 20, 126, 127, 200):
        for H in (1, 20, 256, 257):
            for K in (1, 10, 256, 257):
                for m in (0, 1, 8, 32, 33):
                    ok = lib.xw_tiled_ode_ok(d, H, K, m)
                    assert (lib.xw_paths_tiled_gvjp_work(d, H, K, m) == -1) == (ok == 0), (d, H, K, m)


# ---- host-side refusals, on jobs whose pointers are never dereferenced -------------------------------------------------------------
def _job(**kw):
    job = (_lib.XwPathsGvjpJob * 1)()
    for k in FIELDS[:-1]:
        setattr(job[0], k, 8)                                  # (never dereferenced: every call below is refused on the host)
    job[0].N = 1
    for k, v in kw.items():
        setattr(job[0], k, v)
    return job


def _call(job, njobs=1, theta=8, method=1, L=2, d=3, H=20, K=10, m=8, work=8):
    return _lib.lib.xw_paths_tiled_gvjp(job, njobs, theta, method, L, d, H, K, m, work, None)


def test_host_side_refusals_of_the_entry_point():
    assert _call(None) == E_ARG and _call(_job(), njobs=0) == E_ARG and _call(_job(), njobs=-1) == E_ARG
    assert _call(_job(), theta=None) == E_ARG and _call(_job(), work=None) == E_ARG
    for k in ('xT', 'start', 'tT', 'Y', 'gslab'):
        assert _call(_job(**{k: None})) == E_ARG, k
    # one of vx, vs without the other; a direction without its tangent checkpoints; nothing to differentiate
    assert _call(_job(vx=None)) == E_ARG and _call(_job(vs=None)) == E_ARG and _call(_job(Yd=None)) == E_ARG
    assert _call(_job(wu=None, wt=None, vx=None, vs=None)) == E_ARG
    assert _call(_job(N=0)) == E_ARG and _call(_job(N=-3)) == E_ARG
    assert _call(_job(), L=0) == E_ARG
    for method in (-1, 3, 4):
        assert _call(_job(), method=method) == E_ARG, method
    assert _call(_job(), H=257) == E_DIMS and _call(_job(), K=257) == E_DIMS and _call(_job(), m=33) == E_DIMS
    assert _call(_job(), m=0) == E_DIMS and _call(_job(), d=127) == E_DIMS
    # nstep, wu, wt and the direction with Yd may be NULL (not all of the last three): the refusal is then still the dimension's
    assert _call(_job(nstep=None, wu=None, wt=None), H=257) == E_DIMS
    assert _call(_job(vx=None, vs=None, Yd=None, wt=None), H=257) == E_DIMS
    assert _call(_job(vx=None, vs=None, Yd=None, wu=None), H=257) == E_DIMS


# ---- the chunk bound ----------------------------------------------------------------------------------------------------------------
def test_both_checkpoints_and_slabs_bound_the_chunk():
    budget = EP.EVAL_GRAD_CKPT_BYTES
    for chunk, L, H, d, K in ((65536, 9, 20, 20, 10), (65536, 33, 96, 5, 32), (65536, 9, 256, 5, 256), (1 << 20, 2, 20, 3, 10),
                              (65536, 1 << 20, 256, 5, 256)):
        P = KN.theta_size(d, H, K)
        per = EP.gvjp_chunk_paths(chunk, L, H, P)
        assert per % 16 == 0 and per >= 16 and per <= chunk
        tiles = per // 16
        assert tiles == 1 or 8 * (2 * 16 * L * H + P) * tiles <= budget
        assert per == chunk or 8 * (2 * 16 * L * H + P) * (tiles + 1) > budget               # the largest that fits
        assert per <= EP.vjp_chunk_paths(chunk, L, H, P) and per <= EP.hvp_chunk_paths(chunk, L, H)
    assert EP.gvjp_chunk_paths(65536, 1 << 20, 256, 1000) == 16                              # never below one tile
    assert EP.gvjp_chunk_paths(5, 3, 20, 1000) == 5 and EP.gvjp_chunk_paths(16, 3, 20, 1000) == 16


# ---- the Python surface: every refusal, on CPU tensors, before any launch -----------------------------------------------------------
SETUP = {'dim': 3, 'N_t': 4, 'T0': 0, 'T': 1, 'shape_param': [-1, 1]}
HSETUP = {'dim': 3, 'N_t': 4, 'T0': 0, 'T': 1, 'shape_param': 1.0}
WHO = r'evaluate_grad_vjp\(\)'
LAUNCHES = ('tiled_paths_fwd', 'tiled_paths_grad', 'tiled_paths_hvp', 'tiled_paths_gvjp', 'slab_sum')


def _no_launch(*a, **kw):
    raise AssertionError('a kernel wrapper was called')


def _evaluate(points, wu='ones', wg=None, wt=None, solver='midpoint', domain=sampling.Hypercube, n_sub=None, setup=SETUP,
              chunk=EP.EVAL_CHUNK_PATHS):
    h = lambda X0: X0[:, 1]              # noqa: E731
    if isinstance(wu, str):
        wu = torch.ones(points.shape[0], dtype=F64)
    tail = (n_sub, setup, domain, solver, h, torch.zeros(KN.theta_size(3, 20, 10), dtype=F64), KN.method_id(solver), 20, 10, 8,
            torch.device('cpu'))
    patches = [mock.patch.object(KN, name, _no_launch) for name in LAUNCHES]
    for p in patches:
        p.start()
    try:
        return EP.evaluate_points_grad_vjp(points, wu, wg, wt, *tail, chunk=chunk)
    finally:
        for p in patches:
            p.stop()


@pytest.mark.parametrize('name', ['dopri5', 'explicit_adams'])
def test_the_solvers_without_a_fixed_grid_are_refused(name):
    with pytest.raises(XnwanError, match=WHO) as e:
        _evaluate(torch.zeros(2, 4, dtype=F64), solver=name)
    assert repr(name) in str(e.value) and 'fixed-grid' in str(e.value) and "['euler', 'midpoint', 'rk4']" in str(e.value)


def test_bad_shapes_resolutions_and_domains_are_refused():
    with pytest.raises(XnwanError, match=WHO + r'.*\[M, 4\]'):
        _evaluate(torch.zeros(2, 5, dtype=F64))
    with pytest.raises(XnwanError, match=WHO + '.*n_sub'):
        _evaluate(torch.zeros(2, 4, dtype=F64), n_sub=0)
    with pytest.raises(XnwanError, match='eval_chunk_paths'):
        _evaluate(torch.zeros(2, 4, dtype=F64), chunk=0)

    class Slab:
        pass
    with pytest.raises(XnwanError, match=WHO + '.*Slab.*entry'):
        _evaluate(torch.zeros(2, 4, dtype=F64), domain=Slab)


def test_weights_all_none_or_of_another_shape_are_refused():
    pts = torch.zeros(2, 4, dtype=F64)
    with pytest.raises(XnwanError, match=WHO + '.*at least one of wu'):
        _evaluate(pts, None, None, None)
    for bad in (torch.zeros(2, 1, dtype=F64), torch.zeros(3, dtype=F64), torch.zeros((), dtype=F64), [1.0, 1.0], 1.0):
        with pytest.raises(XnwanError, match=WHO + r': wu must be None or a tensor \[2\]'):
            _evaluate(pts, bad)
        with pytest.raises(XnwanError, match=WHO + r': wt must be None or a tensor \[2\]'):
            _evaluate(pts, None, None, bad)
    for bad in (torch.zeros(2, dtype=F64), torch.zeros(2, 4, dtype=F64), torch.zeros(3, 2, dtype=F64), 1.0):
        with pytest.raises(XnwanError, match=WHO + r': wg must be None or a tensor \[2, 3\]'):
            _evaluate(pts, None, bad)


def test_points_before_their_entry_time_and_re_entered_points_are_refused():
    with pytest.raises(XnwanError, match=WHO + '.*t >= t_in') as e:
        _evaluate(torch.tensor([[0.5, 0.0, 0.0, 0.0], [0.1, 0.0, 0.0, 0.0]], dtype=F64), setup=dict(SETUP, T0=0.25))
    assert '1 points' in str(e.value) and 'point 1' in str(e.value)
    pts = torch.tensor([[0.25, 0.6, 0.0, 0.0], [0.75, 0.3, 0.0, 0.0], [0.75, 0.7, 0.0, 0.0], [0.0, 0.1, 0.2, 0.3]], dtype=F64)
    with pytest.raises(XnwanError, match=WHO + '.*entered at T0') as e:
        _evaluate(pts, domain=sampling.NSphere_THourglass, setup=HSETUP)
    assert '1 points' in str(e.value) and 'point 2' in str(e.value)


def test_an_unbound_module_and_points_that_require_grad_are_refused():
    net = nets.XNODE(20, 1, None, None, SETUP, 10, 8, sampling.Hypercube)
    for call in (lambda: net.evaluate_grad_vjp(torch.zeros(2, 4, dtype=F64), torch.zeros(2, dtype=F64)),
                 lambda: net.evaluate_grad_fn(torch.zeros(2, 4, dtype=F64))):
        with pytest.raises(XnwanError, match=r'bind\(device\) has not been called'):
            call()
    net.bind(torch.device('cpu'))
    with pytest.raises(XnwanError, match=r'evaluate_grad_fn\(\): points that require grad'):
        net.evaluate_grad_fn(torch.zeros(2, 4, dtype=F64, requires_grad=True))
    for name in ('dopri5', 'explicit_adams'):
        other = nets.XNODE(20, 1, None, None, SETUP, 10, 8, sampling.Hypercube, solver=name)
        other.bind(torch.device('cpu'))
        with pytest.raises(XnwanError, match=WHO + '.*' + name):
            other.evaluate_grad_fn(torch.zeros(2, 4, dtype=F64))


def test_no_points_give_exact_zeros():
    r = _evaluate(torch.zeros(0, 4, dtype=F64), torch.zeros(0, dtype=F64), torch.zeros(0, 3, dtype=F64), torch.zeros(0, dtype=F64))
    assert {k: tuple(t.shape) for k, t in r.items()} == {'u': (0,), 'grad': (0, 3), 'ut': (0,), 'gflat': (KN.theta_size(3, 20, 10),)}
    assert all(t.dtype == F64 for t in r.values()) and bool((r['gflat'] == 0).all())
    with pytest.raises(XnwanError, match=WHO + '.*at least one of wu'):
        _evaluate(torch.zeros(0, 4, dtype=F64), None, None, None)


def test_public_surface():
    assert list(inspect.signature(KN.tiled_paths_gvjp).parameters) == ['jobs', 'theta', 'method', 'H', 'K', 'm', 'work']
    assert list(inspect.signature(KN.paths_gvjp_work).parameters) == ['d', 'H', 'K', 'm', 'tiles', 'device']
    assert list(inspect.signature(EP.evaluate_points_grad_vjp).parameters) == [
        'points', 'wu', 'wg', 'wt', 'n_sub', 'setup', 'domain', 'solver', 'h', 'theta', 'method', 'H', 'K', 'm', 'device', 'chunk']
    assert inspect.signature(EP.evaluate_points_grad_vjp).parameters['chunk'].default == EP.EVAL_CHUNK_PATHS
    assert list(inspect.signature(EP.gvjp_chunk_paths).parameters) == ['chunk', 'L', 'H', 'P']
    assert list(inspect.signature(nets.XNODE.evaluate_grad_vjp).parameters) == ['self', 'points', 'wu', 'wg', 'wt', 'n_sub', 'chunk']
    assert list(inspect.signature(nets.XNODE.evaluate_grad_fn).parameters) == ['self', 'points', 'n_sub', 'chunk']
    assert list(inspect.signature(solver.NODE_WAN_solver.evaluate_grad_vjp).parameters) == ['self', 'points', 'wu', 'wg', 'wt', 'n_sub']
    assert issubclass(nets._EvalGradFn, torch.autograd.Function)
    # the existing calls keep their signatures
    assert list(inspect.signature(nets.XNODE.evaluate_vjp).parameters) == ['self', 'points', 'w', 'n_sub', 'chunk']
    assert list(inspect.signature(nets.XNODE.evaluate_fn).parameters) == ['self', 'points', 'n_sub', 'chunk']
    assert list(inspect.signature(nets.XNODE.evaluate_grad).parameters) == ['self', 'points', 'n_sub', 'chunk']
    for fn in (nets.XNODE.evaluate_grad_vjp, solver.NODE_WAN_solver.evaluate_grad_vjp, EP.evaluate_points_grad_vjp, KN.tiled_paths_gvjp):
        doc = ' '.join(fn.__doc__.split())
        assert 'discrete' in doc.lower() and 'held fixed' in doc and 'constants of theta' in doc, fn
    assert 'CONTINUOUS' in nets.XNODE.evaluate_grad_vjp.__doc__ and 'CONTINUOUS' in EP.evaluate_points_grad_vjp.__doc__


# ---- the reference's own floor --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net', range(len(NETS)))
def test_the_oracles_two_routes_agree_far_inside_the_device_bound(net):
    """one path of each network, each method, n in {0, 1, 4} steps: autograd's reverse-over-reverse value of every term of the
    gradient against forward-over-reverse (the tangent of (x, s) -> dU/dtheta), per parameter block, relative to the block's scale
    (measured: 5.0e-15 at worst).  A block that is identically zero in one route is exactly zero in the other.  The floor stays two
    orders inside the device tests' bound of 1e-10."""
    from test_gpu_tiled_stepper import _theta
    d, H, K, m = NETS[net]
    theta, _ = _theta(H, K, m, d, 300 + net)
    g = torch.Generator().manual_seed(40 + net)
    worst = 0.0
    for method in ('euler', 'midpoint', 'rk4'):
        for n in (0, 1, 4):
            x, s = torch.rand(d, generator=g, dtype=F64) * 2 - 1, torch.randn((), generator=g, dtype=F64)
            times = 0.3 * torch.rand((), generator=g, dtype=F64) + torch.cat((torch.zeros(1, dtype=F64),
                                                                              torch.cumsum(0.02 + 0.2 * torch.rand(n, generator=g, dtype=F64), 0)))
            vx, vs = torch.randn(d, generator=g, dtype=F64), torch.randn((), generator=g, dtype=F64)
            rr = O.reverse_over_reverse(theta, m, method, x, s, times, vx, vs)
            fr = O.forward_over_reverse(theta, m, method, x, s, times, vx, vs)
            for term, (A, B) in zip(('u', 'direction', 'ut'), zip(rr, fr)):
                for k in O.U_ORDER:
                    a, b = A[k], B[k]
                    za, zb = bool((a == 0).all()), bool((b == 0).all())
                    assert za == zb, 'identically zero in one route only: %s %s %s n %d' % (term, k, method, n)
                    if za:
                        continue
                    err = float((a - b).abs().max()) / float(a.abs().max())
                    worst = max(worst, err)
                    assert err < FLOOR, '%s %s %s n %d: %.3e' % (term, k, method, n, err)
    print('the oracle\'s floor, %s: %.2e' % (NETS[net], worst))
