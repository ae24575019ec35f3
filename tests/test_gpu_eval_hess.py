"""Hessian-vector products over a ragged group (csrc/xw_tiled_paths_hvp.hip: kt_paths_jvp, kt_paths_hvp) and the second derivatives at
scattered points built on them (kernels.tiled_paths_hvp, evalpaths.evaluate_points_hvp / evaluate_points_hess, evaluate_hvp and
evaluate_hess of XNODE and NODE_WAN_solver) on the device.

Kernel level, inside the guard-banded, poisoned arena of tests/guarded.py (the workspace handed in through work=), at the shapes of
tests/test_gpu_eval_paths.py (its _ragged: a path without a step beside one with L - 1 in one tile; m = 1 puts the tanh factor on
the first pre-activation; H = 65 has a ragged last row block; N = 17 and 37 a ragged last tile; L = 1 no step anywhere), random
directions with a fixed seed:
 (a) every path against oracle.refspec run on that path ALONE: hx, hs by autograd.grad(create_graph=True) and a second grad of
     g . v, ju from g . v, Yd from torch.autograd.functional.jvp of the trajectory -- relative to scale below TOL_G = 1e-10, the
     bound the same block arithmetic is held to in the gradient sweep (the oracle's own double backward agrees with its full Hessian
     times v to 2e-15 of the Hessian's scale: five orders inside the bound);
 (b) a path without a step has hx == 0 and hs == 0 exactly and ju == gs vs to 1e-12;
 (c) every output element and every element of Yd written, no guard element touched, Y, theta and the inputs bit-unchanged;
 (d) the same bits with and without the nstep hint, under a permutation of the paths (directions included), with each of ju, hx, hs
     asked for alone, from a captured-graph replay and in chunks of 16 and 32;
 (e) the d + 1 basis directions assemble a symmetric matrix per path (to TOL_G of its scale), and H (2 v) == 2 (H v) to the bit.
Public surface (f): evaluate_hess and evaluate_hvp on the cube, the cone and the hourglass's T0-entered points against autograd's
Hessian of x -> refspec.u_net([[T0, x] ... [t, x]], h([T0, x])) per point on the CPU."""
import dataclasses
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402
from test_gpu_tiled_stepper import F64, _close, _theta  # noqa: E402
from test_gpu_eval_paths import LS, METHODS, NETS, NS, _eval_points, _ragged, _solver, _theta_of  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_G = 1e-10
OUTS = ('ju', 'hx', 'hs')

_ORACLE = {}


def _directions(N, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, d, generator=g, dtype=F64), torch.randn(N, generator=g, dtype=F64)


def _trajectory(R, theta, m, method, times):
    """(x [1, d], s [1]) -> the states [n + 1, H] of refspec's arithmetic on one path over `times`, the lift as
    tests/test_gpu_eval_grad.py::_oracle_alone writes it"""
    def ys(xi, si):
        s = si.view(-1, 1)
        y0 = torch.relu(torch.relu(s @ theta['IL0_w'].T + theta['IL0_b']) @ theta['IL2_w'].T + theta['IL2_b']) @ theta['IL4_w'].T + theta['IL4_b']
        return R.odeint_fixed(lambda tt, y: R.field(theta, m, xi, tt, y), y0, times, method)[0]
    return ys


def _oracle_alone(theta, H, K, m, method, x, start, n, tT, vx, vs, key):
    """(ju [N], hx [d, N], hs [N], Yd [L, H, N], gs [N]) of every path ALONE over its own n_i + 1 times: g = dU/d(x, s) with its
    graph, ju = g . v, (hx, hs) = d(g . v)/d(x, s) (exact zeros where g . v does not depend on them: no step, gates constants), the
    tangent of the trajectory by torch.autograd.functional.jvp, its last row repeated behind the path's end.  Once per case"""
    if key not in _ORACLE:
        from oracle import refspec as R
        (N, d), L = x.shape, tT.shape[0]
        ju, hx, hs, gs = torch.zeros(N, dtype=F64), torch.zeros(d, N, dtype=F64), torch.zeros(N, dtype=F64), torch.zeros(N, dtype=F64)
        Yd = torch.zeros(L, H, N, dtype=F64)
        theta = {k: v.detach() for k, v in theta.items()}
        for i in range(N):
            ni = int(n[i])
            ys = _trajectory(R, theta, m, method, tT[:ni + 1, i])
            xi = x[i:i + 1].clone().requires_grad_(True)
            si = start[i:i + 1].clone().requires_grad_(True)
            u = (ys(xi, si)[-1:] @ theta['FL_w'].T + theta['FL_b']).reshape(())
            a, b = torch.autograd.grad(u, [xi, si], create_graph=True, allow_unused=True)
            gv = b.reshape(()) * vs[i] + (0.0 if a is None else (a.reshape(-1) * vx[i]).sum())
            ju[i], gs[i] = gv.detach(), b.detach().reshape(())
            if gv.requires_grad:
                p, q = torch.autograd.grad(gv, [xi, si], allow_unused=True)
                hx[:, i] = 0.0 if p is None else p.reshape(-1)
                hs[i] = 0.0 if q is None else q.reshape(())
            _, yd = torch.autograd.functional.jvp(ys, (x[i:i + 1], start[i:i + 1]), (vx[i:i + 1], vs[i:i + 1]))
            Yd[:ni + 1, :, i], Yd[ni + 1:, :, i] = yd, yd[-1]
        _ORACLE[key] = (ju, hx, hs, Yd, gs)
    return _ORACLE[key]


def _forward(KN, arena, blob, x, start, tT, nstep, H, K, m, mid):
    """the guarded forward launch whose checkpoints the launches read: the job with u and Y"""
    L, N = tT.shape
    job = dict(xT=arena.inp(x.t(), name='xT'), start=arena.inp(start, name='start'), tT=arena.inp(tT, name='tT'),
               u=arena.out(L, N, name='u'), Y=arena.out(L, H, N, name='Y'))
    if nstep is not None:
        job['nstep'] = nstep.to(torch.int32).to(arena.device)
    KN.tiled_paths_fwd([job], blob, mid, H, K, m)
    return job


def _hvp(KN, arena, blob, fj, vxT, vs, H, K, m, mid, hint=True, want=OUTS):
    """one guarded launch on the forward job fj with the direction (vxT [d, N], vs [N], views of the arena): the job with Yd, the
    outputs asked for and its guarded workspace"""
    d, N = fj['xT'].shape
    L = fj['tT'].shape[0]
    job = {k: fj[k] for k in ('xT', 'start', 'tT', 'Y')}
    if hint and 'nstep' in fj:
        job['nstep'] = fj['nstep']
    job.update(vx=vxT, vs=vs, Yd=arena.out(L, H, N, name='Yd'))
    for k in want:
        job[k] = arena.out(*((d, N) if k == 'hx' else (N,)), name=k)
    job['work'] = arena.out(KN.lib.xw_paths_tiled_hvp_work(d, H, K, m) * ((N + 15) // 16), name='hvp_work')
    KN.tiled_paths_hvp([{k: v for k, v in job.items() if k != 'work'}], blob, mid, H, K, m, work=job['work'])
    return job


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('net', range(len(NETS)))
@pytest.mark.parametrize('method', METHODS)
def test_per_path_hvp(method, net, N):
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m = NETS[net]
    mid = KN.method_id(method)
    theta, blob_h = _theta(H, K, m, d, 300 + net)
    dev = torch.device('cuda')
    worst = 0.0
    for L in LS:
        seed = 1000 * net + 10 * N + L
        x, start, n, tT = _ragged(N, L, d, seed)
        vx, vs = _directions(N, d, seed + 2)
        if L == 5 and N > 1:
            assert int(n[0]) == 0 and int(n[1]) == 4                 # no step beside four, in one tile
        arena = G.Arena(dev)
        with arena.workspaces(KN):
            blob = arena.inp(blob_h, name='theta')
            fj = _forward(KN, arena, blob, x, start, tT, n, H, K, m, mid)
            vxT, vsd = arena.inp(vx.t(), name='vx'), arena.inp(vs, name='vs')
            torch.cuda.synchronize()
            kept = {k: fj[k].clone() for k in ('xT', 'start', 'tT', 'Y', 'nstep')}
            kept.update(theta=blob.clone(), vx=vxT.clone(), vs=vsd.clone())
            gs = arena.out(N, name='gs')
            KN.tiled_paths_grad([dict({k: fj[k] for k in ('xT', 'start', 'tT', 'Y', 'nstep')}, gs=gs)], blob, mid, H, K, m)
            plain = _hvp(KN, arena, blob, fj, vxT, vsd, H, K, m, mid, hint=False)
            hinted = _hvp(KN, arena, blob, fj, vxT, vsd, H, K, m, mid)
            alone = {k: _hvp(KN, arena, blob, fj, vxT, vsd, H, K, m, mid, want=(k,)) for k in OUTS}
            gen = torch.Generator().manual_seed(seed + 1)
            perm = torch.randperm(N, generator=gen)
            fm = _forward(KN, arena, blob, x[perm], start[perm], tT[:, perm].contiguous(), n[perm], H, K, m, mid)
            moved = _hvp(KN, arena, blob, fm, arena.inp(vx[perm].t(), name='vx'), arena.inp(vs[perm], name='vs'), H, K, m, mid)
        # (c) every output element and every element of Yd written, no guard element touched; Y, theta and the inputs unchanged
        jobs = [plain, hinted, moved] + list(alone.values())
        arena.check(written=[j[k] for j in jobs for k in OUTS + ('Yd',) if k in j] + [fj['u'], fj['Y'], fm['Y'], gs])
        what = '%s %s N %d L %d' % (method, NETS[net], N, L)
        for k in ('xT', 'start', 'tT', 'Y', 'nstep'):
            assert torch.equal(fj[k], kept[k]), '%s changed: %s' % (k, what)
        assert torch.equal(blob, kept['theta']) and torch.equal(vxT, kept['vx']) and torch.equal(vsd, kept['vs']), what
        # (a) every path against the oracle on that path alone
        ju_ref, hx_ref, hs_ref, Yd_ref, gs_ref = _oracle_alone(theta, H, K, m, method, x, start, n, tT, vx, vs, (method, net, N, L))
        for k, ref in (('ju', ju_ref), ('hx', hx_ref), ('hs', hs_ref), ('Yd', Yd_ref)):
            scale = float(ref.abs().max())
            err = float((plain[k].cpu() - ref).abs().max()) / scale if scale > 0 else float(plain[k].abs().max())
            worst = max(worst, err)
            print('%s %s: rel-to-scale error %.3e (scale %.3e)' % (k, what, err, scale))
        _close(plain['ju'], ju_ref, TOL_G, 'ju ' + what)
        _close(plain['Yd'], Yd_ref, TOL_G, 'Yd ' + what)
        if L > 1:
            assert float(hx_ref.abs().max()) > 0 and float(hs_ref.abs().max()) > 0     # (not a comparison of zeros)
            _close(plain['hx'], hx_ref, TOL_G, 'hx ' + what)
            _close(plain['hs'], hs_ref, TOL_G, 'hs ' + what)
        # (b) no step: no curvature, and the directional derivative is the lift's alone
        still = n.to(dev) == 0
        assert bool((plain['hx'][:, still] == 0).all()) and bool((plain['hs'][still] == 0).all()), 'no step, no Hessian: ' + what
        if bool(still.any()):
            want = (gs * vsd)[still]
            assert float((plain['ju'][still] - want).abs().max()) <= 1e-12 * float(want.abs().max()), 'ju == gs vs without a step: ' + what
        _close(gs, gs_ref, TOL_G, 'gs ' + what)
        # (d) the same bits with the nstep hint, with each output alone, beside other tile neighbours
        pd = perm.to(dev)
        for k in OUTS:
            assert torch.equal(hinted[k], plain[k]), 'nstep %s %s' % (k, what)
            assert torch.equal(alone[k][k], plain[k]), 'alone %s %s' % (k, what)
            assert torch.equal(moved[k], plain[k][..., pd]), 'permuted %s %s' % (k, what)
        for j, tag in ((hinted, 'nstep'), (alone['ju'], 'ju alone'), (alone['hx'], 'hx alone'), (alone['hs'], 'hs alone')):
            assert torch.equal(j['Yd'], plain['Yd']), '%s Yd %s' % (tag, what)
        assert torch.equal(moved['Yd'], plain['Yd'][:, :, pd]), 'permuted Yd ' + what
    print('largest rel-to-scale error of %s %s N %d: %.3e' % (method, NETS[net], N, worst))


def _launches(KN, job, blob, H, K, m, mid, lo=0, hi=None):
    """forward and hvp on the paths lo .. hi of the device job (fresh buffers): dict(ju, hx, hs, Yd)"""
    d, N = job['xT'].shape
    hi = N if hi is None else hi
    L, k, dev = job['tT'].shape[0], hi - lo, blob.device
    new = lambda *s: torch.empty(*s, dtype=F64, device=dev)      # noqa: E731
    part = dict(xT=job['xT'][:, lo:hi].contiguous(), start=job['start'][lo:hi].contiguous(), tT=job['tT'][:, lo:hi].contiguous(),
                nstep=job['nstep'][lo:hi].contiguous(), u=new(L, k), Y=new(L, H, k))
    KN.tiled_paths_fwd([part], blob, mid, H, K, m)
    out = dict(ju=new(k), hx=new(d, k), hs=new(k), Yd=new(L, H, k))
    KN.tiled_paths_hvp([dict(part, vx=job['vx'][:, lo:hi].contiguous(), vs=job['vs'][lo:hi].contiguous(), **out)], blob, mid, H, K, m)
    return part, out


def test_graph_replay_and_chunking_give_the_same_bits():
    """37 paths in chunks of 16 and of 32 give the bits of one launch; a captured launch replays to the same bits"""
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m = NETS[2]
    N, L = 37, 5
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 7)
    x, start, n, tT = _ragged(N, L, d, 8)
    vx, vs = _directions(N, d, 9)
    bc = blob.to(dev)
    job = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), tT=tT.to(dev), nstep=n.to(torch.int32).to(dev),
               vx=vx.t().contiguous().to(dev), vs=vs.to(dev))
    part, first = _launches(KN, job, bc, H, K, m, 2)
    for chunk in (16, 32):
        for lo in range(0, N, chunk):
            hi = min(lo + chunk, N)
            _, got = _launches(KN, job, bc, H, K, m, 2, lo, hi)
            for k in OUTS + ('Yd',):
                assert torch.equal(got[k], first[k][..., lo:hi]), (chunk, lo, k)
    full = dict(part, vx=job['vx'], vs=job['vs'], **{k: torch.empty_like(v) for k, v in first.items()})
    work = KN.paths_hvp_work(d, H, K, m, (N + 15) // 16, dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        KN.tiled_paths_hvp([full], bc, 2, H, K, m, work=work)       # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in OUTS + ('Yd',):
        full[k].fill_(float('nan'))
    with torch.cuda.graph(g):
        KN.tiled_paths_hvp([full], bc, 2, H, K, m, work=work)
    g.replay()
    torch.cuda.synchronize()
    for k in OUTS + ('Yd',):
        assert torch.equal(full[k], first[k]), k


@pytest.mark.parametrize('method', METHODS)
def test_basis_directions_assemble_a_symmetric_matrix_and_scaling_by_two_is_exact(method):
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m = NETS[0]
    N, L = 17, 5
    mid = KN.method_id(method)
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 300)
    x, start, n, tT = _ragged(N, L, d, 31)
    bc = blob.to(dev)
    job = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), tT=tT.to(dev), nstep=n.to(torch.int32).to(dev))
    rows = []
    for k in range(d + 1):                                        # e_0 .. e_{d-1} in x, then the start value
        job['vx'] = torch.zeros(d, N, dtype=F64, device=dev)
        job['vs'] = torch.zeros(N, dtype=F64, device=dev)
        (job['vx'][k] if k < d else job['vs']).fill_(1.0)
        _, out = _launches(KN, job, bc, H, K, m, mid)
        rows.append(torch.cat((out['hx'], out['hs'].view(1, N)), 0))
    Hm = torch.stack(rows, 0)                                     # [d + 1, d + 1, N]: row k = H e_k
    scale = float(Hm.abs().max())
    assert scale > 0
    asym = float((Hm - Hm.transpose(0, 1)).abs().max()) / scale
    print('%s: asymmetry %.3e of the Hessian scale %.3e' % (method, asym, scale))
    assert asym < TOL_G
    vx, vs = _directions(N, d, 32)
    job['vx'], job['vs'] = vx.t().contiguous().to(dev), vs.to(dev)
    _, one = _launches(KN, job, bc, H, K, m, mid)
    job['vx'], job['vs'] = 2 * job['vx'], 2 * job['vs']
    _, two = _launches(KN, job, bc, H, K, m, mid)
    for k in OUTS + ('Yd',):
        assert torch.equal(two[k], 2 * one[k]), k
    # ... and the random direction's product is the matrix applied to it
    v = torch.cat((vx.t(), vs.view(1, N)), 0).to(dev)             # [d + 1, N]
    _close(torch.cat((one['hx'], one['hs'].view(1, N)), 0), torch.einsum('kjn,kn->jn', Hm, v), TOL_G, 'H v from the basis ' + method)


def test_kernel_wrapper_refusals():
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    d, H, K, m = NETS[0]
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 1)
    bc = blob.to(dev)
    x, start, n, tT = _ragged(5, 3, d, 2)
    z = lambda *s: torch.zeros(*s, dtype=F64, device=dev)         # noqa: E731
    job = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), tT=tT.to(dev), Y=z(3, H, 5), vx=z(d, 5), vs=z(5), Yd=z(3, H, 5),
               hs=z(5))
    for mid in (KN.DOPRI5, KN.ADAMS):
        with pytest.raises(XnwanError, match='fixed-grid'):
            KN.tiled_paths_hvp([job], bc, mid, H, K, m)
    with pytest.raises(XnwanError, match='nstep'):
        KN.tiled_paths_hvp([dict(job, nstep=n.to(dev))], bc, 0, H, K, m)                           # (int64: the kernel reads int32)
    for k in ('Y', 'vx', 'vs', 'Yd'):
        with pytest.raises(XnwanError, match=k + r'.* is needed'):
            KN.tiled_paths_hvp([{q: v for q, v in job.items() if q != k}], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='no output'):
        KN.tiled_paths_hvp([{k: v for k, v in job.items() if k != 'hs'}], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='vx must have shape'):
        KN.tiled_paths_hvp([dict(job, vx=z(5, d))], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='Yd must have shape'):
        KN.tiled_paths_hvp([dict(job, Yd=z(H, 5))], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='work must have shape'):
        KN.tiled_paths_hvp([job], bc, 0, H, K, m, work=z(7))


# ---- the public surface ----------------------------------------------------------------------------------------------------------------
def _reference(points, params, theta, P, n_sub):
    """per point, on the CPU: n = max(1, ceil((t - T0) / step)) equal steps ending at t; u, its gradient and autograd's Hessian of
    x -> refspec.u_net([[T0, x] ... [t, x]], h([T0, x])): (u [M], grad [M, d], hess [M, d, d])"""
    from oracle import refspec as R
    T0, T = params['T0'], params['T']
    u, grad, hess = [], [], []
    for p in points:
        t = float(p[0])
        n = 0 if t == T0 else max(1, math.ceil((t - T0) / ((T - T0) / n_sub)))
        grid = torch.tensor([T0 + (t - T0) * k / n for k in range(n)] + [t], dtype=F64)

        def U(x):
            X = torch.cat((grid.view(1, -1, 1), x.view(1, 1, -1).expand(1, n + 1, -1)), 2)
            return R.u_net(theta, params, X, P.func_h(X[:, 0, :]).reshape(-1)).reshape(-1)[-1]
        x = p[1:].clone().requires_grad_(True)
        ui = U(x)
        gi, = torch.autograd.grad(ui, x)
        u.append(ui.detach())
        grad.append(gi)
        hess.append(torch.autograd.functional.hessian(U, p[1:].clone()))
    return torch.stack(u), torch.stack(grad), torch.stack(hess)


def _check_surface(S, pts, params, theta, P, what):
    M, d = pts.shape[0], pts.shape[1] - 1
    v = torch.randn(M, d, generator=torch.Generator().manual_seed(41), dtype=F64)
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()[1].copy())
    hs = S.evaluate_hess(pts)
    hv = S.evaluate_hvp(pts, v)
    assert torch.equal(torch.get_rng_state(), rng[0]) and torch.equal(torch.cuda.get_rng_state(), rng[1])
    assert (np.random.get_state()[1] == rng[2]).all()
    g = S.evaluate_grad(pts)
    assert set(hs) == {'u', 'grad', 'hess', 'lap'} and set(hv) == {'u', 'grad', 'dv', 'hvp'}
    assert hs['hess'].shape == (M, d, d) and hs['lap'].shape == (M,) and hv['hvp'].shape == (M, d) and hv['dv'].shape == (M,)
    assert all(t.dtype == F64 and t.is_cuda and not t.requires_grad for t in list(hs.values()) + list(hv.values()))
    for r in (hs, hv):
        assert torch.equal(r['u'], g['u']) and torch.equal(r['grad'], g['grad']), what      # evaluate_grad's bits
    u_ref, g_ref, h_ref = _reference(pts, params, theta, P, params['N_t'])
    assert float(h_ref.abs().max()) > 0
    _close(hs['u'], u_ref, 1e-12, 'u ' + what)
    _close(hs['grad'], g_ref, TOL_G, 'grad ' + what)
    _close(hs['hess'], h_ref, TOL_G, 'hess ' + what)
    assert torch.equal(hs['lap'], torch.diagonal(hs['hess'], dim1=1, dim2=2).sum(1)), what
    _close(hs['lap'], torch.diagonal(h_ref, dim1=1, dim2=2).sum(1), TOL_G, 'lap ' + what)
    vd = v.cuda()
    _close(hv['hvp'], torch.einsum('mkj,mk->mj', hs['hess'], vd), TOL_G, 'hvp == hess @ v ' + what)
    _close(hv['hvp'], torch.einsum('mkj,mk->mj', h_ref, v), TOL_G, 'hvp ' + what)
    _close(hv['dv'], (g_ref * v).sum(1), TOL_G, 'dv ' + what)
    asym = float((hs['hess'] - hs['hess'].transpose(1, 2)).abs().max()) / float(hs['hess'].abs().max())
    print('%s: asymmetry of hess %.3e of its scale' % (what, asym))
    assert asym < TOL_G
    # another resolution, device input, the module's own entry points; chunks of 16 paths: the same bits
    r5 = S.u_net.module.evaluate_hess(pts.cuda(), n_sub=5)
    _close(r5['hess'], _reference(pts, params, theta, P, 5)[2], TOL_G, 'hess n_sub 5 ' + what)
    assert torch.equal(S.u_net.module.evaluate_hvp(pts, v)['hvp'], hv['hvp'])
    S.options = dataclasses.replace(S.options, eval_chunk_paths=16)
    for k, t in S.evaluate_hess(pts).items():
        assert torch.equal(t, hs[k]), k
    for k, t in S.evaluate_hvp(pts, v).items():
        assert torch.equal(t, hv[k]), k
    # an empty cloud
    e = S.evaluate_hess(pts[:0])
    assert e['hess'].shape == (0, d, d) and e['lap'].shape == (0,) and e['hess'].is_cuda
    assert S.evaluate_hvp(pts[:0], v[:0])['hvp'].shape == (0, d)


@pytest.mark.parametrize('domain,funcs,method', [('Hypercube', 'Ex4_1', 'midpoint'), ('NSphere_TCone', 'Ex4_3', 'rk4')])
def test_solver_evaluate_hess_on_the_cube_and_the_cone(domain, funcs, method):
    import importlib
    from xnode_wan_pde_solver_amd._lib import XnwanError
    P = importlib.import_module('configs.%s_funcs' % funcs)
    S, params = _solver(domain, P, method=method)
    pts = _eval_points(domain)
    _check_surface(S, pts, params, _theta_of(S, 8), P, domain)
    with pytest.raises(XnwanError, match=r'evaluate_hvp\(\): v must be a tensor \[M, d\] = \[37, 3\]'):
        S.evaluate_hvp(pts, torch.zeros(37, 4, dtype=F64))
    with pytest.raises(XnwanError, match=r'evaluate_hess\(\).*\[M, 4\]'):
        S.evaluate_hess(pts[:, :3])
    if domain == 'Hypercube':
        early = pts.clone()
        early[9, 0] = -0.25
        with pytest.raises(XnwanError, match=r'evaluate_hess\(\).*t >= t_in') as e:
            S.evaluate_hess(early)
        assert '1 points' in str(e.value) and 'point 9' in str(e.value)


@pytest.mark.parametrize('solver', ['dopri5', 'explicit_adams'])
def test_solvers_without_a_fixed_grid_are_refused(solver):
    import configs.Ex4_1_funcs as P
    from xnode_wan_pde_solver_amd._lib import XnwanError
    S, _ = _solver('Hypercube', P, method=solver)
    pts = _eval_points('Hypercube')
    with pytest.raises(XnwanError, match=r'evaluate_hess\(\): solver %r is not served' % solver):
        S.evaluate_hess(pts)
    with pytest.raises(XnwanError, match=r'evaluate_hvp\(\): solver %r is not served' % solver):
        S.evaluate_hvp(pts, torch.zeros(37, 3, dtype=F64))


def test_a_domain_class_without_entry_is_refused():
    import configs.Ex4_1_funcs as P
    from xnode_wan_pde_solver_amd._lib import XnwanError
    S, _ = _solver('Hypercube', P)

    class Slab:
        pass
    S.u_net.module.domain = Slab
    with pytest.raises(XnwanError, match=r'evaluate_hess\(\): the domain class Slab has no entry'):
        S.evaluate_hess(_eval_points('Hypercube'))


def test_solver_evaluate_hess_on_the_hourglass():
    """the points entered at T0 are served; the cloud with its re-entered points is refused, with the count and the first index"""
    import configs.Ex4_3_funcs as P
    from xnode_wan_pde_solver_amd import sampling
    from xnode_wan_pde_solver_amd._lib import XnwanError
    S, params = _solver('NSphere_THourglass', P, method='euler')
    pts = _eval_points('NSphere_THourglass')
    _, at_T0 = sampling.NSphere_THourglass.entry(pts, 1.0, 0, 1)
    late = (~at_T0).nonzero().view(-1)
    assert at_T0[2] and not at_T0[3] and 0 < late.numel() < 37 and int((pts[at_T0, 0] >= 0.5).sum()) > 0
    _check_surface(S, pts[at_T0].contiguous(), params, _theta_of(S, 8), P, 'hourglass')
    for call in (lambda: S.evaluate_hess(pts), lambda: S.evaluate_hvp(pts, torch.zeros(37, 3, dtype=F64))):
        with pytest.raises(XnwanError, match='entered at T0') as e:
            call()
        assert '%d points' % late.numel() in str(e.value) and 'point %d,' % int(late[0]) in str(e.value)
    assert S.evaluate(pts).shape == (37,)                        # (evaluate() serves the whole cloud, as before)
