"""The reverse sweep over a ragged group (csrc/xw_tiled_paths_grad.hip: kt_paths_grad) and the gradient at scattered points built on
it (kernels.tiled_paths_grad, evalpaths.evaluate_points_grad, XNODE.evaluate_grad, NODE_WAN_solver.evaluate_grad) on the device.

Kernel level, inside the guard-banded, poisoned arena of tests/guarded.py, at the shapes of tests/test_gpu_eval_paths.py (its
_ragged: a path without a step beside one with L - 1 in one tile): every path against oracle.refspec run on that path ALONE under
autograd with respect to its x and its start value (gx, gs relative to scale below 1e-10, the bound tests/test_gpu_tiled_stepper.py
holds the same sweep arithmetic to; ut = FL_w . field(t_end, x, y_final) below 1e-12, the forward's bound); every output element
written, nothing else touched, Y and the inputs bit-unchanged; the same bits with and without the nstep hint, under a permutation of
the paths, with each output asked for alone, from a captured-graph replay and in chunks; the fixed-grid sweep's values
(kernels.tiled_ode_bwd_multi, a separate kernel text: 1e-12, not bits) on a shared grid.  Public surface: solver.evaluate_grad on
the cube, the cone and the hourglass's T0-entered points against a per-point CPU reference built from oracle.refspec.u_net with
autograd through x and through the start value h([T0, x])."""
import dataclasses
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402
from test_gpu_tiled_stepper import F64, _cfg, _close, _theta  # noqa: E402
from test_gpu_eval_paths import LS, METHODS, NETS, NS, _ragged, _theta_of  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_G, TOL_T = 1e-10, 1e-12
OUTS = ('gx', 'gs', 'ut')

_ORACLE = {}


def _oracle_alone(theta, H, K, m, method, x, start, n, tT, key):
    """(gx [d, N], gs [N], ut [N]): refspec's arithmetic on every path ALONE over its own n_i + 1 times, autograd of its final u with
    respect to its x and its start value; ut from refspec.field at the path's last time and final state.  Computed once per case"""
    if key not in _ORACLE:
        from oracle import refspec as R
        N, d = x.shape
        gx, gs, ut = torch.zeros(d, N, dtype=F64), torch.zeros(N, dtype=F64), torch.zeros(N, dtype=F64)
        theta = {k: v.detach() for k, v in theta.items()}
        for i in range(N):
            ni = int(n[i])
            xi = x[i:i + 1].clone().requires_grad_(True)
            si = start[i:i + 1].clone().requires_grad_(True)
            s = si.view(-1, 1)
            y0 = torch.relu(torch.relu(s @ theta['IL0_w'].T + theta['IL0_b']) @ theta['IL2_w'].T + theta['IL2_b']) @ theta['IL4_w'].T + theta['IL4_b']
            ys = R.odeint_fixed(lambda tt, y: R.field(theta, m, xi, tt, y), y0, tT[:ni + 1, i], method)[0]          # [ni + 1, H]
            u = (ys @ theta['FL_w'].T + theta['FL_b']).reshape(-1)[-1]
            Xi = torch.cat((tT[:ni + 1, i].view(1, -1, 1), x[i].view(1, 1, -1).expand(1, ni + 1, -1)), 2)
            assert torch.equal(u.detach(), R.u_net(theta, _cfg(H, K, m, method), Xi, start[i:i + 1]).reshape(-1)[-1])   # the specification
            a, b = torch.autograd.grad(u, [xi, si], allow_unused=True)
            gx[:, i] = 0.0 if a is None else a.reshape(-1)       # (no step: u does not depend on x)
            gs[i] = b.reshape(())
            ut[i] = (R.field(theta, m, x[i:i + 1], tT[ni, i], ys[-1:].detach()) @ theta['FL_w'].T).reshape(())
        _ORACLE[key] = (gx, gs, ut)
    return _ORACLE[key]


def _forward(KN, arena, blob, x, start, tT, nstep, H, K, m, mid):
    """the guarded forward launch whose checkpoints the sweep reads: the job with u and Y"""
    L, N = tT.shape
    job = dict(xT=arena.inp(x.t(), name='xT'), start=arena.inp(start, name='start'), tT=arena.inp(tT, name='tT'),
               u=arena.out(L, N, name='u'), Y=arena.out(L, H, N, name='Y'))
    if nstep is not None:
        job['nstep'] = nstep.to(torch.int32).to(arena.device)
    KN.tiled_paths_fwd([job], blob, mid, H, K, m)
    return job


def _grad(KN, arena, blob, fj, H, K, m, mid, hint=True, want=OUTS):
    """one guarded launch of the sweep on the forward job fj: the job with the outputs asked for"""
    d, N = fj['xT'].shape
    job = {k: fj[k] for k in ('xT', 'start', 'tT', 'Y')}
    if hint and 'nstep' in fj:
        job['nstep'] = fj['nstep']
    for k in want:
        job[k] = arena.out(*((d, N) if k == 'gx' else (N,)), name=k)
    KN.tiled_paths_grad([job], blob, mid, H, K, m)
    return job


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('net', range(len(NETS)))
@pytest.mark.parametrize('method', METHODS)
def test_per_path_sweep(method, net, N):
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
            fj = _forward(KN, arena, blob, x, start, tT, n, H, K, m, mid)
            torch.cuda.synchronize()
            kept = {k: fj[k].clone() for k in ('xT', 'start', 'tT', 'Y', 'nstep')}
            kept['theta'] = blob.clone()
            plain = _grad(KN, arena, blob, fj, H, K, m, mid, hint=False)
            hinted = _grad(KN, arena, blob, fj, H, K, m, mid)
            alone = {k: _grad(KN, arena, blob, fj, H, K, m, mid, want=(k,)) for k in OUTS}
            gen = torch.Generator().manual_seed(seed + 1)
            perm = torch.randperm(N, generator=gen)
            fm = _forward(KN, arena, blob, x[perm], start[perm], tT[:, perm].contiguous(), n[perm], H, K, m, mid)
            moved = _grad(KN, arena, blob, fm, H, K, m, mid)
            # (d) one grid for all paths: the fixed-grid sweep's values under a cotangent that is 1 on the last row
            t_one = tT[:, 1 if N > 1 else 0].contiguous()
            fs = _forward(KN, arena, blob, x, start, t_one.view(L, 1).expand(L, N).contiguous(), None, H, K, m, mid)
            shared = _grad(KN, arena, blob, fs, H, K, m, mid, want=('gx', 'gs'))
            ubar = torch.zeros(L, N, dtype=F64)
            ubar[L - 1] = 1.0
            bj = dict(xT=fs['xT'], start=fs['start'], Y=fs['Y'], ubar=arena.inp(ubar, name='ubar'), gx=arena.out(d, N, name='gx1'),
                      gs=arena.out(N, name='gs1'))
            KN.tiled_ode_bwd_multi([bj], arena.inp(t_one, name='t'), blob, mid, H, K, m, want_x=True, want_params=False)
        # (b) every output element written, no guard element touched; Y and the inputs hold the bits they held
        jobs = [plain, hinted, moved, shared, bj] + list(alone.values())
        arena.check(written=[j[k] for j in jobs for k in OUTS if k in j] + [fj['u'], fj['Y'], fm['Y'], fs['Y']])
        what = '%s %s N %d L %d' % (method, NETS[net], N, L)
        for k in ('xT', 'start', 'tT', 'Y', 'nstep'):
            assert torch.equal(fj[k], kept[k]), '%s changed: %s' % (k, what)
        assert torch.equal(blob, kept['theta']), what
        # (a) every path against the oracle on that path alone
        gx_ref, gs_ref, ut_ref = _oracle_alone(theta, H, K, m, method, x, start, n, tT, (method, net, N, L))
        _close(plain['gx'], gx_ref, TOL_G, 'gx ' + what)
        _close(plain['gs'], gs_ref, TOL_G, 'gs ' + what)
        _close(plain['ut'], ut_ref, TOL_T, 'ut ' + what)
        assert bool((plain['gx'][:, n.to(dev) == 0] == 0).all()), 'a path without a step has no x gradient: ' + what
        # (c) the same bits with the nstep hint, with each output alone, beside other tile neighbours
        pd = perm.to(dev)
        for k in OUTS:
            assert torch.equal(hinted[k], plain[k]), 'nstep %s %s' % (k, what)
            assert torch.equal(alone[k][k], plain[k]), 'alone %s %s' % (k, what)
            assert torch.equal(moved[k], plain[k][..., pd]), 'permuted %s %s' % (k, what)
        # (d)
        _close(shared['gx'], bj['gx'], TOL_T, 'shared grid gx ' + what)
        _close(shared['gs'], bj['gs'], TOL_T, 'shared grid gs ' + what)


def _sweep_in_chunks(KN, job, blob, H, K, m, mid, chunk):
    """the job cut into launches of `chunk` paths (forward and sweep): the outputs put together again"""
    d, N = job['xT'].shape
    L = job['tT'].shape[0]
    dev = blob.device
    out = dict(gx=torch.empty(d, N, dtype=F64, device=dev), gs=torch.empty(N, dtype=F64, device=dev), ut=torch.empty(N, dtype=F64, device=dev))
    for lo in range(0, N, chunk):
        hi = min(lo + chunk, N)
        part = dict(xT=job['xT'][:, lo:hi].contiguous(), start=job['start'][lo:hi].contiguous(), tT=job['tT'][:, lo:hi].contiguous(),
                    nstep=job['nstep'][lo:hi].contiguous(), u=torch.empty(L, hi - lo, dtype=F64, device=dev),
                    Y=torch.empty(L, H, hi - lo, dtype=F64, device=dev))
        KN.tiled_paths_fwd([part], blob, mid, H, K, m)
        g = dict(gx=torch.empty(d, hi - lo, dtype=F64, device=dev), gs=out['gs'][lo:hi], ut=out['ut'][lo:hi])
        KN.tiled_paths_grad([dict(part, **g)], blob, mid, H, K, m)
        out['gx'][:, lo:hi] = g['gx']
    return out


def test_graph_replay_and_chunking_give_the_same_bits():
    """a captured launch replays to the same bits; 37 paths in chunks of 16 and of 32 give the bits of one launch"""
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m = NETS[2]
    N, L = 37, 5
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 7)
    x, start, n, tT = _ragged(N, L, d, 8)
    bc = blob.to(dev)
    job = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), tT=tT.to(dev), nstep=n.to(torch.int32).to(dev),
               u=torch.empty(L, N, dtype=F64, device=dev), Y=torch.empty(L, H, N, dtype=F64, device=dev),
               gx=torch.empty(d, N, dtype=F64, device=dev), gs=torch.empty(N, dtype=F64, device=dev), ut=torch.empty(N, dtype=F64, device=dev))
    KN.tiled_paths_fwd([job], bc, 2, H, K, m)
    KN.tiled_paths_grad([job], bc, 2, H, K, m)
    first = {k: job[k].clone() for k in OUTS}
    for chunk in (16, 32):
        got = _sweep_in_chunks(KN, job, bc, H, K, m, 2, chunk)
        for k in OUTS:
            assert torch.equal(got[k], first[k]), (chunk, k)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        KN.tiled_paths_grad([job], bc, 2, H, K, m)             # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in OUTS:
        job[k].fill_(float('nan'))
    with torch.cuda.graph(g):
        KN.tiled_paths_grad([job], bc, 2, H, K, m)
    g.replay()
    torch.cuda.synchronize()
    for k in OUTS:
        assert torch.equal(job[k], first[k]), k


def test_kernel_wrapper_refusals():
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    d, H, K, m = NETS[0]
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 1)
    bc = blob.to(dev)
    x, start, n, tT = _ragged(5, 3, d, 2)
    job = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), tT=tT.to(dev), Y=torch.zeros(3, H, 5, dtype=F64, device=dev),
               gs=torch.empty(5, dtype=F64, device=dev))
    for mid in (KN.DOPRI5, KN.ADAMS):
        with pytest.raises(XnwanError, match='fixed-grid'):
            KN.tiled_paths_grad([job], bc, mid, H, K, m)
    with pytest.raises(XnwanError, match='nstep'):
        KN.tiled_paths_grad([dict(job, nstep=n.to(dev))], bc, 0, H, K, m)                      # (int64: the kernel reads int32)
    with pytest.raises(XnwanError, match='Y must have shape'):
        KN.tiled_paths_grad([dict(job, Y=torch.zeros(H, 5, dtype=F64, device=dev))], bc, 0, H, K, m)   # (a last_only forward's)
    with pytest.raises(XnwanError, match='Y'):
        KN.tiled_paths_grad([{k: v for k, v in job.items() if k != 'Y'}], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='no output'):
        KN.tiled_paths_grad([{k: v for k, v in job.items() if k != 'gs'}], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='gx must have shape'):
        KN.tiled_paths_grad([dict(job, gx=torch.empty(5, d, dtype=F64, device=dev))], bc, 0, H, K, m)


# ---- the public surface ----------------------------------------------------------------------------------------------------------------
D = 4


def _solver(domain, P, method, seed=11):
    from src.training import NODE_WAN_solver
    params = {'alpha': 1e3, 'u_layers': 8, 'u_hidden_dim': 20, 'u_hidden_hidden_dim': 10, 'v_layers': 2, 'v_hidden_dim': 50,
              'n1': 1, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': method,
              'dim': D, 'N_t': 6, 'N_r': 32, 'N_b': 16, 'T0': 0, 'T': 1, 'shape_param': [-1, 1] if domain == 'Hypercube' else 1.0,
              'iterations': 1, 'domain': domain}
    torch.manual_seed(seed)
    np.random.seed(seed)
    S = NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, torch.device('cuda'), './',
                        func_u_sol=P.func_u_sol, p=2)
    with torch.no_grad():                                        # non-zero biases: every bias path is exercised
        for p in S.u_net.parameters():
            if p.dim() == 1:
                p.copy_(0.3 * torch.randn(p.shape, dtype=F64))
    return S, params


def _points(domain, M=50, seed=21):
    """float64 points [M, 1 + D] inside the domain and entered at T0, with t = T0, t = T and duplicates"""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(M, generator=g, dtype=F64)
    t[0], t[1] = 0.0, 1.0
    if domain == 'Hypercube':
        x = torch.rand(M, D, generator=g, dtype=F64) * 2 - 1
    else:
        z = torch.randn(M, D, generator=g, dtype=F64)
        z = z / z.norm(dim=1, keepdim=True)
        if domain == 'NSphere_TCone':
            bound = 1 - t
        else:                                                    # the hourglass: the narrowing half, or inside the inner ball
            bound = torch.where(t < 0.5, 1 - t, torch.full_like(t, 0.5))
        x = z * (bound * (0.05 + 0.9 * torch.rand(M, generator=g, dtype=F64))).view(M, 1)
    pts = torch.cat((t.view(M, 1), x), 1)
    pts[7], pts[M - 1] = pts[3], pts[3]                          # duplicates, far apart in the cloud
    return pts


def _reference(points, params, theta, P, n_sub):
    """per point, on the CPU: n = max(1, ceil((t - T0) / step)) equal steps ending at t, refspec.u_net on the one-path group with
    start = func_h([T0, x]), autograd through x on both ways; ut from refspec.field at (t, x, y_final): (u, grad, ut)"""
    from oracle import refspec as R
    T0, T, m = params['T0'], params['T'], params['u_layers']
    u, grad, ut = [], [], []
    for p in points:
        t = float(p[0])
        x = p[1:].clone().requires_grad_(True)
        n = 0 if t == T0 else max(1, math.ceil((t - T0) / ((T - T0) / n_sub)))
        grid = torch.tensor([T0 + (t - T0) * k / n for k in range(n)] + [t], dtype=F64)
        X = torch.cat((grid.view(1, -1, 1), x.view(1, 1, -1).expand(1, n + 1, -1)), 2)
        s = P.func_h(X[:, 0, :]).reshape(-1)
        ui = R.u_net(theta, params, X, s).reshape(-1)[-1]
        gi, = torch.autograd.grad(ui, x)
        with torch.no_grad():
            sv = s.view(-1, 1)
            y = torch.relu(torch.relu(sv @ theta['IL0_w'].T + theta['IL0_b']) @ theta['IL2_w'].T + theta['IL2_b']) @ theta['IL4_w'].T + theta['IL4_b']
            xd = x.detach().view(1, -1)
            if n:
                y = R.odeint_fixed(lambda tt, yy: R.field(theta, m, xd, tt, yy), y, grid, params['solver'])[:, -1]
            assert abs(float((y @ theta['FL_w'].T + theta['FL_b']).reshape(()) - ui)) <= 1e-14 * max(1.0, abs(float(ui)))   # (the same state)
            ut.append((R.field(theta, m, xd, grid[-1], y) @ theta['FL_w'].T).reshape(()))
        u.append(ui.detach())
        grad.append(gi)
    return torch.stack(u), torch.stack(grad), torch.stack(ut)


def _check(r, ref, M, what):
    assert set(r) == {'u', 'grad', 'ut'}
    assert r['u'].shape == (M,) and r['grad'].shape == (M, D) and r['ut'].shape == (M,)
    assert all(v.dtype == F64 and v.is_cuda and not v.requires_grad for v in r.values())
    _close(r['u'], ref[0], TOL_T, 'u ' + what)
    _close(r['grad'], ref[1], TOL_G, 'grad ' + what)
    _close(r['ut'], ref[2], TOL_T, 'ut ' + what)


@pytest.mark.parametrize('domain,funcs,method', [('Hypercube', 'Ex4_1', 'midpoint'), ('NSphere_TCone', 'Ex4_3', 'rk4')])
def test_solver_evaluate_grad_on_the_cube_and_the_cone(domain, funcs, method):
    import importlib
    P = importlib.import_module('configs.%s_funcs' % funcs)
    S, params = _solver(domain, P, method)
    theta = _theta_of(S, 8)
    pts = _points(domain)
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()[1].copy())
    r = S.evaluate_grad(pts)
    assert torch.equal(torch.get_rng_state(), rng[0]) and torch.equal(torch.cuda.get_rng_state(), rng[1])
    assert (np.random.get_state()[1] == rng[2]).all()
    assert torch.equal(r['u'], S.evaluate(pts))                  # the forward's bits
    _check(r, _reference(pts, params, theta, P, params['N_t']), 50, '%s default n_sub' % domain)
    assert torch.equal(r['grad'][7], r['grad'][3]) and torch.equal(r['grad'][49], r['grad'][3]) and torch.equal(r['ut'][49], r['ut'][3])
    # another resolution; device input; the module's own entry point
    r5 = S.u_net.module.evaluate_grad(pts.cuda(), n_sub=5)
    assert torch.equal(r5['u'], S.evaluate(pts.cuda(), n_sub=5))  # (the same input: device points get their grids on the device)
    _check(r5, _reference(pts, params, theta, P, 5), 50, '%s n_sub 5' % domain)
    # chunks of 16 paths: the same bits
    S.options = dataclasses.replace(S.options, eval_chunk_paths=16)
    r16 = S.evaluate_grad(pts)
    for k in r:
        assert torch.equal(r16[k], r[k]), k


def test_solver_evaluate_grad_on_the_hourglass():
    """a cloud of points entered at T0 is served; one re-entered point in it is refused, with the count and its index"""
    import configs.Ex4_3_funcs as P
    from xnode_wan_pde_solver_amd import sampling
    from xnode_wan_pde_solver_amd._lib import XnwanError
    S, params = _solver('NSphere_THourglass', P, 'euler')
    theta = _theta_of(S, 8)
    pts = _points('NSphere_THourglass')
    _, at_T0 = sampling.NSphere_THourglass.entry(pts, 1.0, 0, 1)
    assert bool(at_T0.all()) and int((pts[:, 0] >= 0.5).sum()) > 5
    r = S.evaluate_grad(pts)
    assert torch.equal(r['u'], S.evaluate(pts))
    _check(r, _reference(pts, params, theta, P, params['N_t']), 50, 'hourglass')
    bad = pts.clone()
    bad[11, 0] = 0.75
    bad[11, 1:] = torch.tensor([0.7, 0.0, 0.0, 0.0], dtype=F64)  # left the inner ball, came back through the boundary at 0.7
    with pytest.raises(XnwanError, match='entered at T0') as e:
        S.evaluate_grad(bad)
    assert '1 points' in str(e.value) and 'point 11' in str(e.value)
    assert S.evaluate(bad).shape == (50,)                        # (evaluate() serves it, as before)
