"""The per-path forward pass of the tiled family (csrc/xw_tiled_paths.hip: kt_ode_fwd_pp) and the evaluation at scattered points
built on it (kernels.tiled_paths_fwd, Engine.predict_paths, NODE_WAN_solver.evaluate) on the device.

Kernel level, inside the guard-banded, poisoned arena of tests/guarded.py: every path against oracle.refspec run on that path ALONE
(its own grid; u and Y relative to scale below 1e-12, the bound tests/test_gpu_tiled_stepper.py holds the same arithmetic to); the
bits of kernels.tiled_ode_fwd on a shared grid; padded rows equal to the final row; a path's bits independent of its tile
neighbours (a permutation of the paths), of the nstep hint, of a captured-graph replay and of the chunking; every output element
written and nothing else touched.  Public surface: solver.evaluate on the three domains against a per-point CPU reference built from
oracle.refspec.u_net with the same callables (below 1e-12), and Engine.predict_paths on the stacked [[x0, x]] recipe row by row."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402
from test_gpu_tiled_stepper import F64, U_ORDER, _cfg, _close, _theta  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12
METHODS = ('euler', 'midpoint', 'rk4')
NETS = ((3, 20, 10, 8), (20, 65, 16, 1), (5, 96, 32, 8))          # (d, H, K, m); (20, 10): an MFMA container's widths
NS, LS = (1, 15, 16, 17, 37), (1, 2, 5)


def _ragged(N, L, d, seed):
    """x [N, d], start [N], steps n [N] (path 0 takes none, path 1 all L - 1: neighbours in one tile) and the packed grids
    tT [L, N]: every path from a start time of its own over increments of its own, its last time repeated"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(N, d, generator=g) * 2 - 1).double()
    start = torch.randn(N, dtype=F64, generator=g)
    n = torch.randint(0, L, (N,), generator=g)
    n[0] = 0
    if N > 1:
        n[1] = L - 1
    else:
        n[0] = L - 1
    t0 = 0.5 * torch.rand(N, generator=g, dtype=F64)
    inc = 0.02 + 0.2 * torch.rand(L, N, generator=g, dtype=F64)
    inc[0] = 0.0
    inc = inc * (torch.arange(L).view(L, 1) <= n.view(1, N))
    return x, start, n, (t0.view(1, N) + torch.cumsum(inc, 0)).contiguous()


_ORACLE = {}


def _oracle_alone(theta, H, K, m, method, x, start, n, tT, key):
    """(u [L, N], Y [L, H, N]): refspec.u_net's arithmetic on every path ALONE over its own n_i + 1 times, the later rows its final
    value; computed once per case and shared"""
    if key not in _ORACLE:
        from oracle import refspec as R
        L, N = tT.shape
        u, Y = torch.empty(L, N, dtype=F64), torch.empty(L, H, N, dtype=F64)
        cfg = _cfg(H, K, m, method)
        theta = {k: v.detach() for k, v in theta.items()}
        for i in range(N):
            ni = int(n[i])
            s = start[i:i + 1].view(-1, 1)
            y0 = torch.relu(torch.relu(s @ theta['IL0_w'].T + theta['IL0_b']) @ theta['IL2_w'].T + theta['IL2_b']) @ theta['IL4_w'].T + theta['IL4_b']
            ys = R.odeint_fixed(lambda tt, y: R.field(theta, m, x[i:i + 1], tt, y), y0, tT[:ni + 1, i], method)[0]   # [ni + 1, H]
            Xi = torch.cat((tT[:ni + 1, i].view(1, -1, 1), x[i].view(1, 1, -1).expand(1, ni + 1, -1)), 2)
            ui = R.u_net(theta, cfg, Xi, start[i:i + 1]).reshape(-1)                                              # the specification
            assert torch.equal(ui, (ys @ theta['FL_w'].T + theta['FL_b']).reshape(-1))
            u[:ni + 1, i], u[ni + 1:, i] = ui, ui[-1]
            Y[:ni + 1, :, i], Y[ni + 1:, :, i] = ys, ys[-1]
        _ORACLE[key] = (u, Y)
    return _ORACLE[key]


def _launch(KN, arena, blob, x, start, tT, nstep, H, K, m, mid, last_only=False, want_Y=True):
    """one guarded launch: the job with its outputs"""
    L, N = tT.shape
    job = dict(xT=arena.inp(x.t(), name='xT'), start=arena.inp(start, name='start'), tT=arena.inp(tT, name='tT'),
               u=arena.out(*((N,) if last_only else (L, N)), name='u'))
    if want_Y:
        job['Y'] = arena.out(*((H, N) if last_only else (L, H, N)), name='Y')
    if nstep is not None:
        job['nstep'] = nstep.to(torch.int32).to(arena.device)
    KN.tiled_paths_fwd([job], blob, mid, H, K, m, last_only=last_only)
    return job


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('net', range(len(NETS)))
@pytest.mark.parametrize('method', METHODS)
def test_per_path_forward(method, net, N):
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m = NETS[net]
    mid = KN.method_id(method)
    theta, blob_h = _theta(H, K, m, d, 300 + net)
    dev = torch.device('cuda')
    for L in LS:
        seed = 1000 * net + 10 * N + L
        x, start, n, tT = _ragged(N, L, d, seed)
        if L == 5 and N > 1:
            assert int(n[0]) == 0 and int(n[1]) == 4                 # no step beside four, in one tile
        arena = G.Arena(dev)
        with arena.workspaces(KN):
            blob = arena.inp(blob_h, name='theta')
            plain = _launch(KN, arena, blob, x, start, tT, None, H, K, m, mid)
            hinted = _launch(KN, arena, blob, x, start, tT, n, H, K, m, mid)
            last = _launch(KN, arena, blob, x, start, tT, n, H, K, m, mid, last_only=True)
            last_u = _launch(KN, arena, blob, x, start, tT, None, H, K, m, mid, last_only=True, want_Y=False)
            gen = torch.Generator().manual_seed(seed + 1)
            perm = torch.randperm(N, generator=gen)
            moved = _launch(KN, arena, blob, x[perm], start[perm], tT[:, perm].contiguous(), n[perm], H, K, m, mid)
            # (b) one grid for all paths: kt_ode_fwd's bits
            t_one = tT[:, 1 if N > 1 else 0].contiguous()
            shared = _launch(KN, arena, blob, x, start, t_one.view(L, 1).expand(L, N).contiguous(), None, H, K, m, mid)
            fj = dict(xT=shared['xT'], start=shared['start'], u=arena.out(L, N, name='u1'), Y=arena.out(L, H, N, name='Y1'))
            KN.tiled_ode_fwd_multi([fj], arena.inp(t_one, name='t'), blob, mid, H, K, m)
        # (f) every output element written, no guard element touched
        jobs = (plain, hinted, last, last_u, moved, shared, fj)
        arena.check(written=[j[k] for j in jobs for k in ('u', 'Y') if k in j])
        what = '%s %s N %d L %d' % (method, NETS[net], N, L)
        # (a) every path against the oracle on that path alone
        u_ref, Y_ref = _oracle_alone(theta, H, K, m, method, x, start, n, tT, (method, net, N, L))
        _close(plain['u'], u_ref, TOL, 'u ' + what)
        _close(plain['Y'], Y_ref, TOL, 'Y ' + what)
        assert torch.equal(shared['u'], fj['u']) and torch.equal(shared['Y'], fj['Y']), 'shared grid ' + what
        # (c) padded rows hold the final row's bits
        rows = n.to(dev).view(1, N).expand(L, N)
        assert torch.equal(plain['u'], torch.gather(plain['u'], 0, torch.minimum(torch.arange(L, device=dev).view(L, 1), rows))), what
        idx = torch.minimum(torch.arange(L, device=dev).view(L, 1, 1), n.to(dev).view(1, 1, N)).expand(L, H, N)
        assert torch.equal(plain['Y'], torch.gather(plain['Y'], 0, idx)), what
        # (e) the same bits with the nstep hint; last_only: the final row
        assert torch.equal(hinted['u'], plain['u']) and torch.equal(hinted['Y'], plain['Y']), 'nstep ' + what
        assert torch.equal(last['u'], plain['u'][L - 1]) and torch.equal(last['Y'], plain['Y'][L - 1]), 'last_only ' + what
        assert torch.equal(last_u['u'], plain['u'][L - 1]), 'last_only without nstep ' + what
        # (d) other tile neighbours: the same bits per path
        assert torch.equal(moved['u'], plain['u'][:, perm.to(dev)]) and torch.equal(moved['Y'], plain['Y'][:, :, perm.to(dev)]), what


def test_graph_replay_and_chunking_give_the_same_bits():
    """(g) a captured launch replays to the same bits; (h) 37 paths in chunks of 32 give the bits of one launch"""
    from xnode_wan_pde_solver_amd import kernels as KN, evalpaths as EP
    d, H, K, m = NETS[2]
    N, L = 37, 5
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 7)
    x, start, n, tT = _ragged(N, L, d, 8)
    bc, xT, sc, tc, nc = blob.to(dev), x.t().contiguous().to(dev), start.to(dev), tT.to(dev), n.to(torch.int32).to(dev)
    u, Y = torch.empty(L, N, dtype=F64, device=dev), torch.empty(L, H, N, dtype=F64, device=dev)
    job = dict(xT=xT, start=sc, tT=tc, nstep=nc, u=u, Y=Y)
    KN.tiled_paths_fwd([job], bc, 2, H, K, m)
    first = (u.clone(), Y.clone())
    one = EP.paths_forward(xT, tc, sc, nc, bc, 2, H, K, m)
    assert torch.equal(one, first[0])
    assert torch.equal(EP.paths_forward(xT, tc, sc, nc, bc, 2, H, K, m, chunk=32), one)
    assert torch.equal(EP.paths_forward(xT, tc, sc, None, bc, 2, H, K, m, last_only=True, chunk=16), one[L - 1])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        KN.tiled_paths_fwd([job], bc, 2, H, K, m)              # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    u.fill_(float('nan'))
    Y.fill_(float('nan'))
    with torch.cuda.graph(g):
        KN.tiled_paths_fwd([job], bc, 2, H, K, m)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(u, first[0]) and torch.equal(Y, first[1])


def test_kernel_wrapper_refusals():
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    d, H, K, m = NETS[0]
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 1)
    x, start, n, tT = _ragged(5, 3, d, 2)
    job = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), tT=tT.to(dev), u=torch.empty(3, 5, dtype=F64, device=dev))
    for mid in (KN.DOPRI5, KN.ADAMS):
        with pytest.raises(XnwanError, match='fixed-grid'):
            KN.tiled_paths_fwd([job], blob.to(dev), mid, H, K, m)
    with pytest.raises(XnwanError, match='nstep'):
        KN.tiled_paths_fwd([dict(job, nstep=n.to(dev))], blob.to(dev), 0, H, K, m)             # (int64: the kernel reads int32)
    with pytest.raises(XnwanError, match='u must have shape'):
        KN.tiled_paths_fwd([job], blob.to(dev), 0, H, K, m, last_only=True)
    with pytest.raises(XnwanError, match='tT'):
        KN.tiled_paths_fwd([dict(job, tT=tT.t().contiguous().to(dev))], blob.to(dev), 0, H, K, m)


# ---- the public surface ----------------------------------------------------------------------------------------------------------------
def _solver(domain, P, H=20, K=10, m=8, method='midpoint', options=None, seed=11):
    from src.training import NODE_WAN_solver
    params = {'alpha': 1e3, 'u_layers': m, 'u_hidden_dim': H, 'u_hidden_hidden_dim': K, 'v_layers': 2, 'v_hidden_dim': 50,
              'n1': 1, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': method,
              'dim': 3, 'N_t': 6, 'N_r': 32, 'N_b': 16, 'T0': 0, 'T': 1, 'shape_param': [-1, 1] if domain == 'Hypercube' else 1.0,
              'iterations': 1, 'domain': domain}
    torch.manual_seed(seed)
    np.random.seed(seed)
    S = NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, torch.device('cuda'), './',
                        func_u_sol=P.func_u_sol, p=2, options=options)
    with torch.no_grad():                                        # non-zero biases: every bias path is exercised
        for p in S.u_net.parameters():
            if p.dim() == 1:
                p.copy_(0.3 * torch.randn(p.shape, dtype=F64))
    return S, params


def _theta_of(S, m):
    from oracle import refspec as R
    named = dict(S.u_net.named_parameters())
    theta = {k: named[nm].detach().cpu().clone() for nm, k in R.u_names(m)}
    if m == 1:
        K = theta['Win'].shape[0]
        theta['Wh'], theta['Wh_b'] = torch.zeros(K, K, dtype=F64), torch.zeros(K, dtype=F64)
    return theta


def _eval_points(domain, M=37, seed=21):
    """float64 points [M, 4] inside the domain, with t = T0, t = T and, on the hourglass, both halves and both sides of |x| = r / 2"""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(M, generator=g, dtype=F64)
    t[0], t[1] = 0.0, 1.0
    if domain == 'Hypercube':
        x = torch.rand(M, 3, generator=g, dtype=F64) * 2 - 1
    else:
        z = torch.randn(M, 3, generator=g, dtype=F64)
        z = z / z.norm(dim=1, keepdim=True)
        bound = (1 - t) if domain == 'NSphere_TCone' else torch.where(t <= 0.5, 1 - t, t)
        x = z * (bound * (0.05 + 0.9 * torch.rand(M, generator=g, dtype=F64))).view(M, 1)
        if domain == 'NSphere_THourglass':
            t[2], x[2] = 0.75, 0.3 * z[2]                      # widening half, never left the inner ball: from T0 with h
            t[3], x[3] = 0.75, 0.7 * z[3]                      # ... re-entered at 0.7 with g
            t[4], x[4] = 0.25, 0.6 * z[4]                      # narrowing half, outside the inner ball: from T0
            t[5], x[5] = 0.8, torch.tensor([0.0, 0.8, 0.0], dtype=F64)   # on the moving boundary: t == t_in to the bit
                                                               # (sqrt(0.8 * 0.8 + 0 + 0) == 0.8 in any summation order), no step
            t[1], x[1] = 1.0, 0.9 * z[1]
    return torch.cat((t.view(M, 1), x), 1)


def _reference(points, domain, params, theta, P, n_sub):
    """per point, on the CPU: entry by the domain's rule (restated), n = max(1, ceil((t - t_in) / step)) equal steps ending at t,
    refspec.u_net on the one-path group with the start value of the same callables"""
    from oracle import refspec as R
    T0, T = params['T0'], params['T']
    out = []
    for p in points:
        t, x = float(p[0]), p[1:]
        t_in, boundary = float(T0), False
        if domain == 'NSphere_THourglass':
            rad, half = float(torch.sqrt(torch.sum(x ** 2))), (T - T0) / 2
            if not (t < half or rad <= params['shape_param'] * half):
                t_in, boundary = rad / params['shape_param'], True
        n = 0 if t == t_in else max(1, math.ceil((t - t_in) / ((T - T0) / n_sub)))
        grid = torch.tensor([t_in + (t - t_in) * k / n for k in range(n)] + [t], dtype=F64)
        X = torch.cat((grid.view(1, -1, 1), x.view(1, 1, -1).expand(1, n + 1, -1)), 2)
        s = P.func_g(X[:, :1, :]).reshape(-1) if boundary else P.func_h(X[:, 0, :]).reshape(-1)
        out.append(R.u_net(theta, params, X, s).reshape(-1)[-1])
    return torch.stack(out)


EVAL_CASES = [('Hypercube', 'Ex4_1', 20, 10, 8, 'midpoint'), ('NSphere_TCone', 'Ex4_3', 20, 10, 8, 'rk4'),
              ('NSphere_THourglass', 'Ex4_3', 20, 10, 8, 'euler'), ('NSphere_THourglass', 'Ex4_3', 65, 16, 1, 'midpoint')]


@pytest.mark.parametrize('domain,funcs,H,K,m,method', EVAL_CASES)
def test_solver_evaluate_matches_a_per_point_reference(domain, funcs, H, K, m, method):
    import importlib
    P = importlib.import_module('configs.%s_funcs' % funcs)
    S, params = _solver(domain, P, H, K, m, method)
    theta = _theta_of(S, m)
    pts = _eval_points(domain)
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()[1].copy())
    u = S.evaluate(pts)
    assert u.shape == (37,) and u.dtype == F64 and u.is_cuda and not u.requires_grad
    assert torch.equal(torch.get_rng_state(), rng[0]) and torch.equal(torch.cuda.get_rng_state(), rng[1])
    assert (np.random.get_state()[1] == rng[2]).all()
    _close(u, _reference(pts, domain, params, theta, P, params['N_t']), TOL, 'evaluate %s' % domain)
    # another resolution; device input; the module's own entry point; float32 input is widened exactly
    u3 = S.u_net.module.evaluate(pts.cuda(), n_sub=3)
    _close(u3, _reference(pts, domain, params, theta, P, 3), TOL, 'evaluate %s n_sub 3' % domain)
    p32 = pts.float()
    _close(S.evaluate(p32[6:]), _reference(p32[6:].double(), domain, params, theta, P, params['N_t']), TOL, 'float32 input')
    if domain == 'NSphere_THourglass':
        from xnode_wan_pde_solver_amd import sampling
        t_in, at_T0 = sampling.NSphere_THourglass.entry(pts, params['shape_param'], 0, 1)
        assert at_T0[2] and not at_T0[3] and at_T0[4] and not at_T0[5] and float(t_in[5]) == float(pts[5, 0])


def test_predict_paths_on_the_stacked_readme_recipe():
    """[[x0, x]] per point, stacked to [N, 2, 1 + d]: starters at T0 (h) and on the moving boundary (g) mixed; row by row against
    the oracle on the one-path group; eval_chunk_paths = 32 gives the same bits as one launch"""
    import dataclasses
    import configs.Ex4_3_funcs as P
    from oracle import refspec as R
    from xnode_wan_pde_solver_amd.options import EngineOptions
    S, params = _solver('NSphere_THourglass', P, method='rk4')
    theta = _theta_of(S, 8)
    pts = _eval_points('NSphere_THourglass')
    from xnode_wan_pde_solver_amd import sampling
    t_in, at_T0 = sampling.NSphere_THourglass.entry(pts, 1.0, 0, 1)
    X = torch.stack((torch.cat((t_in.view(-1, 1), pts[:, 1:]), 1), pts), 1)                      # [37, 2, 4]
    assert 0 < int(at_T0.sum()) < 37
    u = S.engine.predict_paths(X)
    assert u.shape == (2, 37)
    want = torch.stack([R.u_net(theta, params, X[i:i + 1], (P.func_h(X[i:i + 1, 0, :]) if at_T0[i] else P.func_g(X[i:i + 1, :1, :])).reshape(-1)).reshape(-1)
                        for i in range(37)], 1)
    _close(u, want, TOL, 'predict_paths')
    S.engine.options = dataclasses.replace(S.engine.options, eval_chunk_paths=32)
    assert torch.equal(S.engine.predict_paths(X), u)
    assert torch.equal(S.engine.predict_paths(X.cuda(), starts=torch.where(at_T0, P.func_h(X[:, 0, :]), P.func_g(X[:, :1, :]).reshape(-1))), u)
    from xnode_wan_pde_solver_amd._lib import XnwanError
    bad = X.clone()
    bad[3, 1, 0] = bad[3, 0, 0] - 0.1
    with pytest.raises(XnwanError, match='must not decrease'):
        S.engine.predict_paths(bad)
