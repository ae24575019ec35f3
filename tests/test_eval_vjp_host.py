"""CPU-side checks of the parameter gradients at scattered points (include/xnwan_vjp.h, csrc/xw_tiled_paths_vjp.hip,
kernels.tiled_paths_vjp / paths_vjp_work, evalpaths.vjp_chunk_paths / evaluate_points_vjp, XNODE.evaluate_vjp / evaluate_fn,
NODE_WAN_solver.evaluate_vjp): the new header against its ctypes table and the library, the older headers and tables as they were,
the workspace query, every host-side refusal of the C entry point, the chunk bound with its slab term, the host chain (sort, chunks,
the sum of the chunks' slabs) with the kernel layer replaced by oracle.refspec's autograd on every path, every refusal of the Python
surface by its message, the empty cloud and the public signatures.  No kernel is launched."""
import contextlib
import inspect
import os
import re
import subprocess
import sys
from unittest import mock

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN, nets, sampling, solver, _lib  # noqa: E402
from xnode_wan_pde_solver_amd._lib import XnwanError  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NAMES = ('xw_paths_tiled_vjp_work', 'xw_paths_tiled_vjp')
FIELDS = ['xT', 'start', 'tT', 'nstep', 'Y', 'w', 'gslab', 'gx', 'gs', 'N']
U_ORDER = ['IL0_w', 'IL0_b', 'IL2_w', 'IL2_b', 'IL4_w', 'IL4_b', 'Win', 'Win_b', 'Wh', 'Wh_b', 'Wo', 'Wo_b', 'FL_w', 'FL_b']
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


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    hdr = _header('xnwan_vjp.h')
    assert '#include "xnwan.h"' in hdr
    assert _declared(hdr) == set(NAMES) == set(_lib.VJP_SIGNATURES)
    out = _exported()
    for name in NAMES:
        args = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')
        assert len(args) == len(_lib.VJP_SIGNATURES[name]), name
        assert re.search(r'\bT\s+' + name + r'\b', out), name
        assert getattr(_lib.lib, name).argtypes == _lib.VJP_SIGNATURES[name]
        assert not name.startswith('xw_tiled_')                 # (tests/test_tiled_stepper_host.py pins that set)
    assert _fields(hdr, 'XwPathsVjpJob') == [f[0] for f in _lib.XwPathsVjpJob._fields_] == FIELDS
    # what is differentiated, and the slab format, are part of the header
    assert 'DISCRETE' in hdr and 'held fixed' in hdr and 'constant of theta' in hdr and 'ReLU gates constants' in hdr
    assert 'xw_tiled_ode_bwd_slabs(N) rows' in hdr and 'xw_slab_sum' in hdr and 'zeroes it on the stream' in hdr


def test_the_kernel_is_in_the_library_and_not_exported():
    blob = open(_lib.LIB_PATH, 'rb').read()
    assert b'kt_paths_vjp' in blob
    assert not re.findall(r'\b[A-Za-z]\s+(\S*kt_paths_vjp\S*)', _exported())


def test_the_older_headers_and_tables_are_as_they_were():
    declared = _declared(_header('xnwan.h'))
    assert len(declared) == 64 and declared == set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 33 == _lib.lib.xw_abi_version()
    assert _declared(_header('xnwan_eval.h')) == {'xw_paths_dopri5_work', 'xw_paths_dopri5_fwd'} == set(_lib.EVAL_SIGNATURES)
    assert _declared(_header('xnwan_grad.h')) == {'xw_paths_tiled_grad_work', 'xw_paths_tiled_grad'} == set(_lib.GRAD_SIGNATURES)
    assert _declared(_header('xnwan_eval_grad.h')) == {'xw_paths_dopri5_ckpt_fwd', 'xw_paths_dopri5_grad_work',
                                                       'xw_paths_dopri5_grad'} == set(_lib.EVAL_GRAD_SIGNATURES)
    assert _declared(_header('xnwan_hess.h')) == {'xw_paths_tiled_hvp_work', 'xw_paths_tiled_hvp'} == set(_lib.HESS_SIGNATURES)
    assert _declared(_header('xnwan_jet.h')) == {'xw_paths_tiled_jet_work', 'xw_paths_tiled_jet'} == set(_lib.JET_SIGNATURES)
    assert [f[0] for f in _lib.XwPathsGradJob._fields_] == ['xT', 'start', 'tT', 'nstep', 'Y', 'gx', 'gs', 'ut', 'N'] \
        == _fields(_header('xnwan_grad.h'), 'XwPathsGradJob')
    older = (declared | set(_lib.EVAL_SIGNATURES) | set(_lib.GRAD_SIGNATURES) | set(_lib.EVAL_GRAD_SIGNATURES) | set(_lib.HESS_SIGNATURES)
             | set(_lib.JET_SIGNATURES) | set(_lib.SWITCH_SIGNATURES))
    assert not set(NAMES) & older


def test_workspace_query():
    """per tile: the gradient sweep's workspace and the 16 stage times behind it; -1 exactly where xw_tiled_ode_ok refuses"""
    lib = _lib.lib
    for d, H, K, m in ((20, 20, 10, 8), (3, 65, 16, 1), (5, 96, 32, 8), (5, 256, 256, 32)):
        got = lib.xw_paths_tiled_vjp_work(d, H, K, m)
        assert got >= lib.xw_paths_tiled_grad_work(d, H, K, m) > 0
        assert got == lib.xw_paths_tiled_grad_work(d, H, K, m) + 16
    for d in (1, 3, 20, 126, 127, 200):
        for H in (1, 20, 256, 257):
            for K in (1, 10, 256, 257):
                for m in (0, 1, 8, 32, 33):
                    ok = lib.xw_tiled_ode_ok(d, H, K, m)
                    assert (lib.xw_paths_tiled_vjp_work(d, H, K, m) == -1) == (ok == 0), (d, H, K, m)
    assert lib.xw_paths_tiled_vjp_work(20, 257, 16, 8) == -1 and lib.xw_paths_tiled_vjp_work(20, 20, 257, 8) == -1
    assert lib.xw_paths_tiled_vjp_work(20, 20, 10, 33) == -1 and lib.xw_paths_tiled_vjp_work(20, 20, 10, 0) == -1


# ---- host-side refusals, on jobs whose pointers are never dereferenced -------------------------------------------------------------
def _job(**kw):
    job = (_lib.XwPathsVjpJob * 1)()
    for k in FIELDS[:-1]:
        setattr(job[0], k, 8)                                  # (never dereferenced: every call below is refused on the host)
    job[0].N = 1
    for k, v in kw.items():
        setattr(job[0], k, v)
    return job


def _call(job, njobs=1, theta=8, method=1, L=2, d=3, H=20, K=10, m=8, work=8):
    return _lib.lib.xw_paths_tiled_vjp(job, njobs, theta, method, L, d, H, K, m, work, None)


def test_host_side_refusals_of_the_entry_point():
    assert _call(None) == E_ARG and _call(_job(), njobs=0) == E_ARG and _call(_job(), njobs=-1) == E_ARG
    assert _call(_job(), theta=None) == E_ARG and _call(_job(), work=None) == E_ARG
    for k in ('xT', 'start', 'tT', 'Y', 'w', 'gslab'):
        assert _call(_job(**{k: None})) == E_ARG, k
    assert _call(_job(N=0)) == E_ARG and _call(_job(N=-3)) == E_ARG
    assert _call(_job(), L=0) == E_ARG
    for method in (-1, 3, 4):
        assert _call(_job(), method=method) == E_ARG, method
    assert _call(_job(), H=257) == E_DIMS and _call(_job(), K=257) == E_DIMS and _call(_job(), m=33) == E_DIMS
    assert _call(_job(), m=0) == E_DIMS and _call(_job(), d=127) == E_DIMS
    # nstep, gx and gs may be NULL: with them missing the refusal is still the dimension's, not the argument's
    assert _call(_job(nstep=None, gx=None, gs=None), H=257) == E_DIMS


# ---- the chunk bound ----------------------------------------------------------------------------------------------------------------
def test_checkpoints_and_slabs_bound_the_chunk():
    budget = EP.EVAL_GRAD_CKPT_BYTES
    for chunk, L, H, d, K in ((65536, 9, 20, 20, 10), (65536, 33, 96, 5, 32), (65536, 9, 256, 5, 256), (1 << 20, 2, 20, 3, 10),
                              (65536, 1 << 20, 256, 5, 256)):
        P = KN.theta_size(d, H, K)
        per = EP.vjp_chunk_paths(chunk, L, H, P)
        assert per % 16 == 0 and per >= 16 and per <= chunk
        tiles = per // 16
        assert tiles == 1 or 8 * (L * H * per + P * tiles) <= budget
        assert per == chunk or 8 * (L * H * (per + 16) + P * (tiles + 1)) > budget            # the largest that fits
        assert per <= EP.grad_chunk_paths(chunk, L, H)                                        # never more than the checkpoints alone allow
    # the slab term dominates at (256, 256): about 2 MB per tile against 16 L H doubles of checkpoints
    P = KN.theta_size(5, 256, 256)
    assert 8 * P > 2_000_000 and P > 4 * 16 * 9 * 256
    assert EP.vjp_chunk_paths(65536, 9, 256, P) == 16 * (budget // (8 * (16 * 9 * 256 + P))) < EP.grad_chunk_paths(65536, 9, 256) // 4
    assert EP.vjp_chunk_paths(65536, 1 << 20, 256, P) == 16                                   # never below one tile
    assert EP.vjp_chunk_paths(5, 3, 20, 1000) == 5 and EP.vjp_chunk_paths(16, 3, 20, 1000) == 16


# ---- the host chain, the kernel layer replaced by autograd on every path ------------------------------------------------------------
def _unflatten(flat, d, H, K):
    """theta's generic layout at (d, H, K) as the oracle's dict (views of flat)"""
    shapes = {'IL0_w': (H, 1), 'IL0_b': (H,), 'IL2_w': (H, H), 'IL2_b': (H,), 'IL4_w': (H, H), 'IL4_b': (H,), 'Win': (K, d + 1 + H),
              'Win_b': (K,), 'Wh': (K, K), 'Wh_b': (K,), 'Wo': (H, K), 'Wo_b': (H,), 'FL_w': (1, H), 'FL_b': (1,)}
    out, off = {}, 0
    for k in U_ORDER:
        n = 1
        for s in shapes[k]:
            n *= s
        out[k] = flat[off:off + n].view(shapes[k])
        off += n
    assert off == flat.numel() == KN.theta_size(d, H, K)
    return out


def _path_u(theta, m, names, mid, x, s, times):
    from oracle import refspec as R
    sv = s.view(-1, 1)
    y0 = torch.relu(torch.relu(sv @ theta['IL0_w'].T + theta['IL0_b']) @ theta['IL2_w'].T + theta['IL2_b']) @ theta['IL4_w'].T + theta['IL4_b']
    ys = R.odeint_fixed(lambda tt, y: R.field(theta, m, x.view(1, -1), tt, y), y0, times, names[mid])[0]
    return (ys[-1:] @ theta['FL_w'].T + theta['FL_b']).reshape(())


def _stubs(m):
    """the contracts of kernels.tiled_paths_fwd / tiled_paths_vjp / slab_sum on the host: per path its final u, and into the slab of
    its tile w_p times autograd's gradient in theta, x and start of oracle.refspec's arithmetic on that path alone"""
    names = {0: 'euler', 1: 'midpoint', 2: 'rk4'}
    calls = []

    def tiled_paths_fwd(jobs, blob, mid, H, K, mm, last_only=False):
        assert not last_only and mm == m
        for j in jobs:
            d, N = j['xT'].shape
            th = _unflatten(blob, d, H, K)
            assert j['Y'].shape == (j['tT'].shape[0], H, N) and j['u'].shape == j['tT'].shape
            for i in range(N):
                ni = int(j['nstep'][i])
                j['u'][:, i] = _path_u(th, m, names, mid, j['xT'][:, i], j['start'][i:i + 1], j['tT'][:ni + 1, i])

    def tiled_paths_vjp(jobs, blob, mid, H, K, mm, work=None):
        with torch.enable_grad():
            for j in jobs:
                d, N = j['xT'].shape
                calls.append(N)
                P = KN.theta_size(d, H, K)
                assert j['gslab'].shape == ((N + 15) // 16, P) and j['w'].shape == (N,) and j['gs'].shape == (N,)
                assert all(j[k].is_contiguous() for k in ('xT', 'tT', 'w', 'gslab'))
                j['gslab'].zero_()
                for i in range(N):
                    ni = int(j['nstep'][i])
                    flat = blob.clone().requires_grad_(True)
                    s = j['start'][i:i + 1].clone().requires_grad_(True)
                    u = _path_u(_unflatten(flat, d, H, K), m, names, mid, j['xT'][:, i], s, j['tT'][:ni + 1, i])
                    g, gs = torch.autograd.grad(u, [flat, s])
                    j['gslab'][i // 16] += j['w'][i] * g
                    j['gs'][i] = j['w'][i] * gs.reshape(())

    def slab_sum(gslab, out=None, accumulate=False):
        assert accumulate and out is not None
        out += gslab.sum(0)
        return out
    return tiled_paths_fwd, tiled_paths_vjp, slab_sum, calls, names


SETUP = {'dim': 3, 'N_t': 4, 'T0': 0, 'T': 1, 'shape_param': [-1, 1]}


def _points(M, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat((torch.rand(M, 1, generator=g, dtype=F64), torch.rand(M, d, generator=g, dtype=F64) * 2 - 1), 1)


@contextlib.contextmanager
def _host_kernels(m):
    fwd, vjp, ssum, calls, names = _stubs(m)
    with mock.patch.object(KN, 'tiled_paths_fwd', fwd), mock.patch.object(KN, 'tiled_paths_vjp', vjp), \
            mock.patch.object(KN, 'slab_sum', ssum):
        yield calls, names


@pytest.mark.parametrize('method', ['euler', 'rk4'])
def test_host_chain_against_autograd_on_every_point(method):
    """evaluate_points_vjp with the launches replaced by the stubs: sort and inverse, chunks of 16 against one chunk, u passed
    through, gflat the weighted sum over the cloud of autograd's gradient of every point's own discrete solution"""
    from test_gpu_tiled_stepper import _theta
    d, H, K, m, M = 3, 20, 10, 8, 20
    _, blob = _theta(H, K, m, d, 5)
    blob = blob.detach()
    h = lambda X0: torch.sin(1.3 * X0[:, 1]) * X0[:, 2] + 0.5 * X0[:, 3] ** 2 + X0[:, 0]              # noqa: E731
    pts = _points(M, d, 12)
    pts[0, 0], pts[1, 0] = 0.0, 1.0                                # no step; the whole interval
    w = torch.randn(M, generator=torch.Generator().manual_seed(13), dtype=F64)
    mid = KN.method_id(method)
    tail = (None, SETUP, sampling.Hypercube, method, h, blob, mid, H, K, m, torch.device('cpu'))
    with _host_kernels(m) as (calls, names):
        r16 = EP.evaluate_points_vjp(pts, w, *tail, chunk=16)
        assert calls == [16, 4]
        one = EP.evaluate_points_vjp(pts, w, *tail)
        assert calls == [16, 4, 20]
        f32 = EP.evaluate_points_vjp(pts.float(), w.float(), *tail)
    assert set(one) == {'u', 'gflat', 'start'} and one['gflat'].shape == (KN.theta_size(d, H, K),)
    assert torch.equal(r16['u'], one['u']) and torch.equal(r16['start'], one['start'])
    scale = float(one['gflat'].abs().max())
    assert scale > 1e-3 and float((r16['gflat'] - one['gflat']).abs().max()) <= 1e-12 * scale
    assert f32['u'].dtype == F64 and f32['gflat'].dtype == F64
    # the reference: every point alone, in the caller's order
    n = EP.step_counts(pts[:, 0], torch.zeros(M, dtype=F64), 0, 1, 4)
    grids = EP.pack_grids(pts[:, 0], torch.zeros(M, dtype=F64), n)
    want, u_ref, gs_ref = torch.zeros_like(blob), [], []
    for i in range(M):
        flat = blob.clone().requires_grad_(True)
        first = torch.cat((torch.zeros(1, 1, dtype=F64), pts[i:i + 1, 1:]), 1)
        s = h(first).clone().requires_grad_(True)
        u = _path_u(_unflatten(flat, d, H, K), m, names, mid, pts[i, 1:], s, grids[:int(n[i]) + 1, i])
        g, gs = torch.autograd.grad(u, [flat, s])
        want += w[i] * g
        u_ref.append(u.detach())
        gs_ref.append(w[i] * gs.reshape(()))
    assert float((one['u'] - torch.stack(u_ref)).abs().max()) <= 1e-13          # u passed through, put back in the caller's order
    assert float((one['start'] - torch.stack(gs_ref)).abs().max()) <= 1e-12 * float(torch.stack(gs_ref).abs().max())
    assert float((one['gflat'] - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_module_level_params_have_the_modules_names_and_shapes():
    """XNODE.evaluate_vjp on a module narrower than its container (a padded blob): params under named_parameters() names, in the
    parameters' shapes, the padding's share exact zeros; no step anywhere gives ZEROS for the field, not None"""
    torch.manual_seed(3)
    h = lambda X0: X0[:, 1] * X0[:, 2] + 0.3                       # noqa: E731
    net = nets.XNODE(18, 1, h, None, SETUP, 9, 3, sampling.Hypercube, solver='midpoint')
    net.bind(torch.device('cpu'))
    Hc, Kc = net.kdims
    assert net.blob.embedded and (Hc, Kc) != (18, 9)
    pts = _points(7, 3, 4)
    w = torch.randn(7, generator=torch.Generator().manual_seed(5), dtype=F64)
    with _host_kernels(3), mock.patch.object(torch.cuda, 'device', lambda dev: contextlib.nullcontext()):
        r = net.evaluate_vjp(pts, w)
        at_T0 = net.evaluate_vjp(torch.cat((torch.zeros(7, 1, dtype=F64), pts[:, 1:]), 1), w)
    named = dict(net.named_parameters())
    assert list(r['params']) == list(named) == net.blob.names and set(r) == {'u', 'params', 'start'}
    for k, p in named.items():
        assert r['params'][k].shape == p.shape and r['params'][k].dtype == F64, k
        assert float(r['params'][k].abs().max()) > 0, k
    for k, g in at_T0['params'].items():
        assert g is not None and g.shape == named[k].shape
        if k.startswith('ODE_rhs.'):
            assert bool((g == 0).all()), k
        else:
            assert float(g.abs().max()) > 0, k


# ---- the Python surface: every refusal, on CPU tensors, before any launch -----------------------------------------------------------
HSETUP = {'dim': 3, 'N_t': 4, 'T0': 0, 'T': 1, 'shape_param': 1.0}
WHO = r'evaluate_vjp\(\)'


def _no_launch(*a, **kw):
    raise AssertionError('a kernel wrapper was called')


def _evaluate(points, w=None, solver='midpoint', domain=sampling.NSphere_THourglass, n_sub=None, setup=HSETUP, chunk=EP.EVAL_CHUNK_PATHS):
    h = lambda X0: X0[:, 1]              # noqa: E731
    if w is None and torch.is_tensor(points):
        w = torch.ones(points.shape[0], dtype=F64)
    tail = (n_sub, setup, domain, solver, h, torch.zeros(KN.theta_size(3, 20, 10), dtype=F64), KN.method_id(solver), 20, 10, 8,
            torch.device('cpu'))
    with mock.patch.object(KN, 'tiled_paths_vjp', _no_launch), mock.patch.object(KN, 'tiled_paths_fwd', _no_launch), \
            mock.patch.object(KN, 'slab_sum', _no_launch):
        return EP.evaluate_points_vjp(points, w, *tail, chunk=chunk)


@pytest.mark.parametrize('solver', ['dopri5', 'explicit_adams'])
def test_the_solvers_without_a_fixed_grid_are_refused(solver):
    with pytest.raises(XnwanError, match=WHO) as e:
        _evaluate(torch.zeros(2, 4, dtype=F64), solver=solver)
    assert repr(solver) in str(e.value) and 'fixed-grid' in str(e.value) and "['euler', 'midpoint', 'rk4']" in str(e.value)
    assert 'no per-path record sweep with slabs or multistep history' in str(e.value)


def test_bad_shapes_resolutions_and_domains_are_refused():
    with pytest.raises(XnwanError, match=WHO + r'.*\[M, 4\]'):
        _evaluate(torch.zeros(2, 5, dtype=F64))
    with pytest.raises(XnwanError, match=r'\[M, 4\]'):
        _evaluate(torch.zeros(4, dtype=F64))
    with pytest.raises(XnwanError, match=WHO + '.*n_sub'):
        _evaluate(torch.zeros(2, 4, dtype=F64), n_sub=0)
    with pytest.raises(XnwanError, match='eval_chunk_paths'):
        _evaluate(torch.zeros(2, 4, dtype=F64), chunk=0)

    class Slab:
        pass
    with pytest.raises(XnwanError, match=WHO + '.*Slab.*entry'):
        _evaluate(torch.zeros(2, 4, dtype=F64), domain=Slab)


def test_weights_of_another_shape_are_refused():
    pts = torch.zeros(2, 4, dtype=F64)
    for w in (torch.zeros(2, 1, dtype=F64), torch.zeros(3, dtype=F64), torch.zeros((), dtype=F64), torch.zeros(1, 2, dtype=F64), [1.0, 1.0], 1.0):
        with pytest.raises(XnwanError, match=WHO + r': w must be a tensor \[M\] = \[2\]'):
            _evaluate(pts, w, domain=sampling.Hypercube, setup=dict(HSETUP, shape_param=[-1, 1]))


def test_points_before_their_entry_time_are_refused():
    with pytest.raises(XnwanError, match=WHO + '.*t >= t_in') as e:
        _evaluate(torch.tensor([[0.5, 0.0, 0.0, 0.0], [0.1, 0.0, 0.0, 0.0]], dtype=F64), domain=sampling.Hypercube,
                  setup=dict(HSETUP, T0=0.25, shape_param=[-1, 1]))
    assert '1 points' in str(e.value) and 'point 1' in str(e.value)


def test_re_entered_hourglass_points_are_refused_with_count_and_index():
    pts = torch.tensor([[0.25, 0.6, 0.0, 0.0], [0.75, 0.3, 0.0, 0.0], [0.75, 0.7, 0.0, 0.0], [0.0, 0.1, 0.2, 0.3],
                        [0.9, 0.0, 0.4, 0.0]], dtype=F64)
    with pytest.raises(XnwanError, match=WHO + '.*entered at T0') as e:
        _evaluate(pts)
    assert '1 points' in str(e.value) and 'point 2' in str(e.value) and 'evaluate_grad()' in str(e.value)
    with pytest.raises(XnwanError, match='2 points'):
        _evaluate(torch.cat((pts, pts[2:3]), 0))


def test_an_unbound_module_and_points_that_require_grad_are_refused():
    net = nets.XNODE(20, 1, None, None, SETUP, 10, 8, sampling.Hypercube)
    for call in (lambda: net.evaluate_vjp(torch.zeros(2, 4, dtype=F64), torch.zeros(2, dtype=F64)),
                 lambda: net.evaluate_fn(torch.zeros(2, 4, dtype=F64))):
        with pytest.raises(XnwanError, match=r'bind\(device\) has not been called'):
            call()
    net.bind(torch.device('cpu'))
    with pytest.raises(XnwanError, match=r'evaluate_fn\(\): points that require grad.*evaluate_grad\(\)'):
        net.evaluate_fn(torch.zeros(2, 4, dtype=F64, requires_grad=True))
    for name in ('dopri5', 'explicit_adams'):
        other = nets.XNODE(20, 1, None, None, SETUP, 10, 8, sampling.Hypercube, solver=name)
        other.bind(torch.device('cpu'))
        with pytest.raises(XnwanError, match=WHO + '.*' + name):
            other.evaluate_fn(torch.zeros(2, 4, dtype=F64))


def test_no_points_give_exact_zeros():
    r = _evaluate(torch.zeros(0, 4, dtype=F64), torch.zeros(0, dtype=F64))
    assert {k: tuple(t.shape) for k, t in r.items()} == {'u': (0,), 'gflat': (KN.theta_size(3, 20, 10),), 'start': (0,)}
    assert all(t.dtype == F64 for t in r.values()) and bool((r['gflat'] == 0).all())


def test_public_surface():
    assert list(inspect.signature(KN.tiled_paths_vjp).parameters) == ['jobs', 'theta', 'method', 'H', 'K', 'm', 'work']
    assert list(inspect.signature(KN.paths_vjp_work).parameters) == ['d', 'H', 'K', 'm', 'tiles', 'device']
    assert list(inspect.signature(EP.evaluate_points_vjp).parameters) == ['points', 'w', 'n_sub', 'setup', 'domain', 'solver', 'h', 'theta',
                                                                          'method', 'H', 'K', 'm', 'device', 'chunk']
    assert inspect.signature(EP.evaluate_points_vjp).parameters['chunk'].default == EP.EVAL_CHUNK_PATHS
    assert list(inspect.signature(EP.vjp_chunk_paths).parameters) == ['chunk', 'L', 'H', 'P']
    assert list(inspect.signature(nets.XNODE.evaluate_vjp).parameters) == ['self', 'points', 'w', 'n_sub', 'chunk']
    assert list(inspect.signature(nets.XNODE.evaluate_fn).parameters) == ['self', 'points', 'n_sub', 'chunk']
    assert list(inspect.signature(solver.NODE_WAN_solver.evaluate_vjp).parameters) == ['self', 'points', 'w', 'n_sub']
    assert issubclass(nets._EvalFn, torch.autograd.Function)
    # the existing calls keep their signatures
    assert list(inspect.signature(nets.XNODE.evaluate).parameters) == ['self', 'points', 'n_sub', 'chunk', 'max_steps']
    assert list(inspect.signature(nets.XNODE.evaluate_grad).parameters) == ['self', 'points', 'n_sub', 'chunk']
    for fn in (nets.XNODE.evaluate_vjp, solver.NODE_WAN_solver.evaluate_vjp, EP.evaluate_points_vjp, KN.tiled_paths_vjp, nets.XNODE.evaluate_fn):
        assert 'discrete' in fn.__doc__.lower() and 'held fixed' in fn.__doc__ and 'constant of theta' in fn.__doc__, fn
    assert 'ZEROS, not None' in nets.XNODE.evaluate_vjp.__doc__
    from xnode_wan_pde_solver_amd.options import EngineOptions
    import dataclasses
    assert not [f.name for f in dataclasses.fields(EngineOptions) if 'vjp' in f.name]
