"""The reverse sweep with slabs over a ragged group (csrc/xw_tiled_paths_vjp.hip: kt_paths_vjp) and the parameter gradients at
scattered points built on it (kernels.tiled_paths_vjp, evalpaths.evaluate_points_vjp, XNODE.evaluate_vjp / evaluate_fn,
NODE_WAN_solver.evaluate_vjp) on the device.

Kernel level, inside the guard-banded, poisoned arena of tests/guarded.py, at the shapes of tests/test_gpu_eval_paths.py (its
_ragged: a path without a step beside one with L - 1 in one tile; every path a start time of its own): slab_sum(gslab), gx and gs
against oracle.refspec run on every path ALONE under autograd in theta, x and start, summed with the weights on the host, below
1e-10 of the scale of each parameter block (the bound tests/test_gpu_eval_grad.py and tests/test_gpu_tiled_stepper.py hold the same
sweep arithmetic to), the time column Win[:, d] a block of its own; every element of gslab, gx, gs written, no guard touched, the
inputs bit-unchanged; the same bits with and without the nstep hint, with gx / gs asked for or not, launched twice, replayed from a
captured graph; (2 w) gives exactly twice every output; a one-hot weight gives the slab sum of that path's own N = 1 launch; w = 0
on the stepless path changes nothing else; gx, gs under a permutation.  Other summation orders or kernel texts -- gflat under a
permutation, chunks of 16 and 32, the fixed-grid sweep on one shared grid, w times tiled_paths_grad's gx, gs -- below 1e-12.
Public surface: solver.evaluate_vjp on the cube, the cone and the hourglass's T0-entered points against a per-point CPU loop over
oracle.refspec.u_net with autograd in theta; evaluate_fn under torch.autograd.grad and torch.optim.SGD; the refusals."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402
from test_gpu_tiled_stepper import F64, U_ORDER, _cfg, _close, _theta  # noqa: E402
from test_gpu_eval_paths import LS, METHODS, NETS, NS, _eval_points, _ragged, _solver, _theta_of  # noqa: E402
from test_gpu_eval_grad import _forward  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_G, TOL_T = 1e-10, 1e-12
_ORACLE = {}


def _weights(N, seed):
    w = torch.randn(N, dtype=F64, generator=torch.Generator().manual_seed(seed))
    assert bool((w != 0).all())
    return w


def _blocks(theta, d):
    """name -> index tensor into the flat gradient (theta's generic layout, U_ORDER), Win cut into its x columns, its time column
    and its y columns"""
    out, off = {}, 0
    for k in U_ORDER:
        n = theta[k].numel()
        idx = torch.arange(off, off + n)
        if k == 'Win':
            idx = idx.view(theta[k].shape)
            out['Win[:, :d]'], out['Win[:, d]'], out['Win[:, d+1:]'] = idx[:, :d].reshape(-1), idx[:, d].reshape(-1), idx[:, d + 1:].reshape(-1)
        else:
            out[k] = idx
        off += n
    return out


def _oracle_alone(theta, H, K, m, method, x, start, n, tT, key):
    """per path, refspec's arithmetic on that path ALONE over its own n_i + 1 times, autograd of its final u in theta, its x and its
    start value: (G [N, P_u], gx [d, N], gs [N]), unweighted.  Computed once per case and left unchanged"""
    if key not in _ORACLE:
        from oracle import refspec as R
        N, d = x.shape
        Gm, gx, gs = [], torch.zeros(d, N, dtype=F64), torch.zeros(N, dtype=F64)
        for i in range(N):
            ni = int(n[i])
            th = {k: v.detach().clone().requires_grad_(True) for k, v in theta.items()}
            xi = x[i:i + 1].clone().requires_grad_(True)
            si = start[i:i + 1].clone().requires_grad_(True)
            s = si.view(-1, 1)
            y0 = torch.relu(torch.relu(s @ th['IL0_w'].T + th['IL0_b']) @ th['IL2_w'].T + th['IL2_b']) @ th['IL4_w'].T + th['IL4_b']
            ys = R.odeint_fixed(lambda tt, y: R.field(th, m, xi, tt, y), y0, tT[:ni + 1, i], method)[0]              # [ni + 1, H]
            u = (ys @ th['FL_w'].T + th['FL_b']).reshape(-1)[-1]
            Xi = torch.cat((tT[:ni + 1, i].view(1, -1, 1), x[i].view(1, 1, -1).expand(1, ni + 1, -1)), 2)
            with torch.no_grad():
                assert torch.equal(u.detach(), R.u_net(th, _cfg(H, K, m, method), Xi, start[i:i + 1]).reshape(-1)[-1])   # the specification
            g = torch.autograd.grad(u, [xi, si] + [th[k] for k in U_ORDER], allow_unused=True)
            gx[:, i] = 0.0 if g[0] is None else g[0].reshape(-1)
            gs[i] = g[1].reshape(())
            Gm.append(torch.cat([(torch.zeros_like(th[k]) if a is None else a).reshape(-1) for k, a in zip(U_ORDER, g[2:])]))
        _ORACLE[key] = (torch.stack(Gm), gx, gs)
    return _ORACLE[key]


def _vjp(KN, arena, blob, fj, w, H, K, m, mid, hint=True, want=('gx', 'gs')):
    """one guarded launch of the sweep on the forward job fj with the weights w (host): the job with its slabs, the outputs asked
    for and the slabs' sum (outside the arena)"""
    d, N = fj['xT'].shape
    tiles = (N + 15) // 16
    job = {k: fj[k] for k in ('xT', 'start', 'tT', 'Y')}
    if hint and 'nstep' in fj:
        job['nstep'] = fj['nstep']
    job['w'] = arena.inp(w, name='w')
    job['gslab'] = arena.out(tiles, blob.numel(), name='gslab')
    for k in want:
        job[k] = arena.out(*((d, N) if k == 'gx' else (N,)), name=k)
    work = arena.out(KN.lib.xw_paths_tiled_vjp_work(d, H, K, m) * tiles, name='vjp_work')
    KN.tiled_paths_vjp([job], blob, mid, H, K, m, work=work)
    job['gflat'] = KN.slab_sum(job['gslab'])
    return job


def _check_blocks(got, ref, blocks, m, L, what, record=None):
    """got against ref block by block, 1e-10 of each block's own scale; a block whose reference is identically zero by construction
    -- the hidden layers' slot of an m = 1 net, the whole field where no path takes a step (L == 1) -- must be exact zeros"""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    for name, idx in blocks.items():
        g, r = got[idx], ref[idx]
        field = name in ('Wh', 'Wh_b', 'Wo', 'Wo_b', 'Win_b') or name.startswith('Win')
        if (m == 1 and name in ('Wh', 'Wh_b')) or (L == 1 and field):
            assert bool((r == 0).all()) and bool((g == 0).all()), 'exact zeros expected: %s %s' % (name, what)
            continue
        scale = float(r.abs().max())
        assert scale > 0, 'a comparison of zeros: %s %s' % (name, what)
        err = float((g - r).abs().max()) / scale
        if record is not None:
            record[name] = max(record.get(name, 0.0), err)
        assert err < TOL_G, '%s %s: max rel-to-scale error %.3e (scale %.3e)' % (name, what, err, scale)


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('net', range(len(NETS)))
@pytest.mark.parametrize('method', METHODS)
def test_per_path_sweep_with_slabs(method, net, N):
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m = NETS[net]
    mid = KN.method_id(method)
    theta, blob_h = _theta(H, K, m, d, 300 + net)
    blocks = _blocks(theta, d)
    dev = torch.device('cuda')
    worst = {}
    for L in LS:
        seed = 1000 * net + 10 * N + L
        x, start, n, tT = _ragged(N, L, d, seed)
        w = _weights(N, seed + 5)
        if L == 5 and N > 1:
            assert int(n[0]) == 0 and int(n[1]) == 4                 # no step beside four, in one tile
            assert float((tT[0] - tT[0, 0]).abs().max()) > 0.01      # a start time per path: a tile-wide t fails the time column
        arena = G.Arena(dev)
        with arena.workspaces(KN):
            blob = arena.inp(blob_h, name='theta')
            fj = _forward(KN, arena, blob, x, start, tT, n, H, K, m, mid)
            torch.cuda.synchronize()
            kept = {k: fj[k].clone() for k in ('xT', 'start', 'tT', 'Y', 'nstep')}
            kept['theta'] = blob.clone()
            plain = _vjp(KN, arena, blob, fj, w, H, K, m, mid, hint=False)
            kept['w'] = plain['w'].clone()
            hinted = _vjp(KN, arena, blob, fj, w, H, K, m, mid)
            bare = _vjp(KN, arena, blob, fj, w, H, K, m, mid, want=())
            only_gs = _vjp(KN, arena, blob, fj, w, H, K, m, mid, want=('gs',))
            again = _vjp(KN, arena, blob, fj, w, H, K, m, mid, hint=False)
            twice = _vjp(KN, arena, blob, fj, 2 * w, H, K, m, mid)
            w0 = w.clone()
            w0[0] = 0.0                                            # (path 0 takes no step where N > 1)
            muted = _vjp(KN, arena, blob, fj, w0, H, K, m, mid)
            perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed + 1))
            fm = _forward(KN, arena, blob, x[perm], start[perm], tT[:, perm].contiguous(), n[perm], H, K, m, mid)
            moved = _vjp(KN, arena, blob, fm, w[perm], H, K, m, mid)
            # the cotangent 1 on every path: w times tiled_paths_grad's gx and gs
            ones = dict({k: fj[k] for k in ('xT', 'start', 'tT', 'Y', 'nstep')}, gx=arena.out(d, N, name='gx1'), gs=arena.out(N, name='gs1'))
            KN.tiled_paths_grad([ones], blob, mid, H, K, m)
            # one grid for all paths: the fixed-grid sweep with its parameter part under ubar = w on the last row
            t_one = tT[:, 1 if N > 1 else 0].contiguous()
            fs = _forward(KN, arena, blob, x, start, t_one.view(L, 1).expand(L, N).contiguous(), None, H, K, m, mid)
            shared = _vjp(KN, arena, blob, fs, w, H, K, m, mid)
            ubar = torch.zeros(L, N, dtype=F64)
            ubar[L - 1] = w
            bj = dict(xT=fs['xT'], start=fs['start'], Y=fs['Y'], ubar=arena.inp(ubar, name='ubar'), gx=arena.out(d, N, name='gxs'),
                      gs=arena.out(N, name='gss'), gslab=arena.out((N + 15) // 16, blob.numel(), name='gslabs'))
            KN.tiled_ode_bwd_multi([bj], arena.inp(t_one, name='t'), blob, mid, H, K, m, want_x=True, want_params=True)
            bj['gflat'] = KN.slab_sum(bj['gslab'])
        # every element of gslab, gx, gs written, no guard element touched (the workspaces' included); the inputs hold their bits
        jobs = [plain, hinted, bare, only_gs, again, twice, muted, moved, shared, bj, ones]
        arena.check(written=[j[k] for j in jobs for k in ('gslab', 'gx', 'gs') if k in j] + [fj['Y'], fm['Y'], fs['Y']])
        what = '%s %s N %d L %d' % (method, NETS[net], N, L)
        for k in ('xT', 'start', 'tT', 'Y', 'nstep'):
            assert torch.equal(fj[k], kept[k]), '%s changed: %s' % (k, what)
        assert torch.equal(blob, kept['theta']) and torch.equal(plain['w'], kept['w']), what
        # the oracle: every path alone, summed with the weights on the host
        Gm, gx_ref, gs_ref = _oracle_alone(theta, H, K, m, method, x, start, n, tT, (method, net, N, L))
        _check_blocks(plain['gflat'], (w.view(-1, 1) * Gm).sum(0), blocks, m, L, what, worst)
        _close(plain['gs'], w * gs_ref, TOL_G, 'gs ' + what)
        if L > 1:
            _close(plain['gx'], w.view(1, -1) * gx_ref, TOL_G, 'gx ' + what)
        assert bool((plain['gx'][:, n.to(dev) == 0] == 0).all()), 'a path without a step has no x gradient: ' + what
        # bits: the hint, the outputs asked for, the same launch twice, twice the weights
        for other, name in ((hinted, 'nstep'), (bare, 'no gx, gs'), (only_gs, 'gs alone'), (again, 'again')):
            assert torch.equal(other['gslab'], plain['gslab']), '%s gslab %s' % (name, what)
            for k in ('gx', 'gs'):
                if k in other:
                    assert torch.equal(other[k], plain[k]), '%s %s %s' % (name, k, what)
        for k in ('gslab', 'gx', 'gs'):
            assert torch.equal(twice[k], 2 * plain[k]), '2 w %s %s' % (k, what)
        # w = 0 on path 0: exact zeros for it, every other path's outputs as they were, the sum still the oracle's
        assert float(muted['gs'][0]) == 0.0 and bool((muted['gx'][:, 0] == 0).all())
        assert torch.equal(muted['gs'][1:], plain['gs'][1:]) and torch.equal(muted['gx'][:, 1:], plain['gx'][:, 1:]), what
        assert torch.equal(muted['gslab'][1:], plain['gslab'][1:]), what
        if N > 1:
            _check_blocks(muted['gflat'], (w0.view(-1, 1) * Gm).sum(0), blocks, m, L, 'w[0] = 0 ' + what)
        # a permutation of the paths with their weights: gx, gs to the bit, the sum in another order
        pd = perm.to(dev)
        for k in ('gx', 'gs'):
            assert torch.equal(moved[k], plain[k][..., pd]), 'permuted %s %s' % (k, what)
        _close(moved['gflat'], plain['gflat'], TOL_T, 'permuted gflat ' + what)
        # other kernel texts
        _close(plain['gx'], w.to(dev).view(1, -1) * ones['gx'], TOL_T, 'w * tiled_paths_grad gx ' + what)
        _close(plain['gs'], w.to(dev) * ones['gs'], TOL_T, 'w * tiled_paths_grad gs ' + what)
        _close(shared['gflat'], bj['gflat'], TOL_T, 'shared grid gflat ' + what)
        _close(shared['gx'], bj['gx'], TOL_T, 'shared grid gx ' + what)
        _close(shared['gs'], bj['gs'], TOL_T, 'shared grid gs ' + what)
    print('largest error against the oracle, %s %s N %d: %.2e' % (method, NETS[net], N, max(worst.values())))


@pytest.mark.parametrize('N', (17, 37))
@pytest.mark.parametrize('method', METHODS)
def test_a_one_hot_weight_gives_that_paths_own_launch(method, N):
    """neighbours and padding lanes add exact zeros: the slab sum under a weight on path i alone is, to the bit, the slab sum of the
    N = 1 launch of that path"""
    from xnode_wan_pde_solver_amd import kernels as KN
    dev = torch.device('cuda')
    L = 5
    for net, (d, H, K, m) in enumerate(NETS):
        mid = KN.method_id(method)
        _, blob_h = _theta(H, K, m, d, 300 + net)
        x, start, n, tT = _ragged(N, L, d, 77 + N + net)
        w = _weights(N, 78 + N)
        arena = G.Arena(dev)
        written = []
        with arena.workspaces(KN):
            blob = arena.inp(blob_h, name='theta')
            fj = _forward(KN, arena, blob, x, start, tT, n, H, K, m, mid)
            for i in (0, 1, 16, N - 1):
                hot = torch.zeros(N, dtype=F64)
                hot[i] = w[i]
                full = _vjp(KN, arena, blob, fj, hot, H, K, m, mid)
                f1 = _forward(KN, arena, blob, x[i:i + 1], start[i:i + 1], tT[:, i:i + 1].contiguous(), n[i:i + 1], H, K, m, mid)
                alone = _vjp(KN, arena, blob, f1, w[i:i + 1], H, K, m, mid)
                written += [full['gslab'], full['gx'], full['gs'], alone['gslab'], alone['gx'], alone['gs'], f1['Y']]
                what = '%s %s N %d path %d' % (method, NETS[net], N, i)
                assert float(alone['gflat'].abs().max()) > 0, what
                assert torch.equal(full['gflat'], alone['gflat']), what
                assert torch.equal(full['gx'][:, i], alone['gx'][:, 0]) and torch.equal(full['gs'][i], alone['gs'][0]), what
                rest = torch.arange(N) != i
                assert bool((full['gs'][rest.to(dev)] == 0).all()) and bool((full['gx'][:, rest.to(dev)] == 0).all()), what
                # the tiles that hold no weight keep the zeros the entry point gave them
                for k in range((N + 15) // 16):
                    if k != i // 16:
                        assert bool((full['gslab'][k] == 0).all()), what
        arena.check(written=written + [fj['Y']])


def _vjp_in_chunks(KN, job, w, blob, H, K, m, mid, chunk):
    """the job cut into launches of `chunk` paths (forward, sweep, slab_sum accumulated): (gflat, gx, gs)"""
    d, N = job['xT'].shape
    L = job['tT'].shape[0]
    dev = blob.device
    new = lambda *shape: torch.empty(*shape, dtype=F64, device=dev)   # noqa: E731
    gflat, gx, gs = torch.zeros(blob.numel(), dtype=F64, device=dev), new(d, N), new(N)
    for lo in range(0, N, chunk):
        hi = min(lo + chunk, N)
        part = dict(xT=job['xT'][:, lo:hi].contiguous(), start=job['start'][lo:hi].contiguous(), tT=job['tT'][:, lo:hi].contiguous(),
                    nstep=job['nstep'][lo:hi].contiguous(), u=new(L, hi - lo), Y=new(L, H, hi - lo))
        KN.tiled_paths_fwd([part], blob, mid, H, K, m)
        g = dict(w=w[lo:hi].contiguous(), gslab=new((hi - lo + 15) // 16, blob.numel()), gx=new(d, hi - lo), gs=gs[lo:hi])
        KN.tiled_paths_vjp([dict(part, **g)], blob, mid, H, K, m)
        KN.slab_sum(g['gslab'], out=gflat, accumulate=True)
        gx[:, lo:hi] = g['gx']
    return gflat, gx, gs


def test_graph_replay_and_chunking():
    """a captured launch (the slabs' zeroing and the sweep) replays to the same bits; 37 paths in chunks of 16 and of 32 give gx, gs
    to the bit and the summed gradient below 1e-12 (another order of the slabs' sum)"""
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m = NETS[2]
    N, L = 37, 5
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 7)
    x, start, n, tT = _ragged(N, L, d, 8)
    bc, w = blob.to(dev), _weights(N, 9).to(dev)
    new = lambda *shape: torch.empty(*shape, dtype=F64, device=dev)   # noqa: E731
    job = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), tT=tT.to(dev), nstep=n.to(torch.int32).to(dev), u=new(L, N),
               Y=new(L, H, N), w=w, gslab=new(3, bc.numel()), gx=new(d, N), gs=new(N))
    work = KN.paths_vjp_work(d, H, K, m, 3, dev)
    KN.tiled_paths_fwd([job], bc, 2, H, K, m)
    KN.tiled_paths_vjp([job], bc, 2, H, K, m, work=work)
    first = {k: job[k].clone() for k in ('gslab', 'gx', 'gs')}
    gflat = KN.slab_sum(job['gslab'])
    for chunk in (16, 32):
        got = _vjp_in_chunks(KN, job, w, bc, H, K, m, 2, chunk)
        _close(got[0], gflat, TOL_T, 'gflat in chunks of %d' % chunk)
        assert torch.equal(got[1], first['gx']) and torch.equal(got[2], first['gs']), chunk
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        KN.tiled_paths_vjp([job], bc, 2, H, K, m, work=work)     # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in first:
        job[k].fill_(float('nan'))
    with torch.cuda.graph(g):
        KN.tiled_paths_vjp([job], bc, 2, H, K, m, work=work)
    g.replay()
    torch.cuda.synchronize()
    for k in first:
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
               w=torch.ones(5, dtype=F64, device=dev), gslab=torch.empty(1, bc.numel(), dtype=F64, device=dev))
    for mid in (KN.DOPRI5, KN.ADAMS):
        with pytest.raises(XnwanError, match='fixed-grid'):
            KN.tiled_paths_vjp([job], bc, mid, H, K, m)
    with pytest.raises(XnwanError, match='nstep'):
        KN.tiled_paths_vjp([dict(job, nstep=n.to(dev))], bc, 0, H, K, m)                       # (int64: the kernel reads int32)
    with pytest.raises(XnwanError, match='Y must have shape'):
        KN.tiled_paths_vjp([dict(job, Y=torch.zeros(H, 5, dtype=F64, device=dev))], bc, 0, H, K, m)    # (a last_only forward's)
    for k in ('Y', 'w', 'gslab'):
        with pytest.raises(XnwanError, match='tiled_paths_vjp: ' + k):
            KN.tiled_paths_vjp([{a: v for a, v in job.items() if a != k}], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='w must have shape'):
        KN.tiled_paths_vjp([dict(job, w=torch.ones(5, 1, dtype=F64, device=dev))], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='w must be torch.float64'):
        KN.tiled_paths_vjp([dict(job, w=torch.ones(5, device=dev))], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='gslab must have shape'):
        KN.tiled_paths_vjp([dict(job, gslab=torch.empty(2, bc.numel(), dtype=F64, device=dev))], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='gslab must be contiguous'):
        KN.tiled_paths_vjp([dict(job, gslab=torch.empty(1, 2 * bc.numel(), dtype=F64, device=dev)[:, ::2])], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='work must have shape'):
        KN.tiled_paths_vjp([job], bc, 0, H, K, m, work=torch.empty(8, dtype=F64, device=dev))


# ---- the public surface ----------------------------------------------------------------------------------------------------------------
M = 37


def _entered_at_T0(domain, params):
    """_eval_points' cloud with the hourglass's re-entered points taken out (M stays 37: the first T0-entered points fill the gaps)"""
    from xnode_wan_pde_solver_amd import sampling
    pts = _eval_points(domain)
    if domain == 'NSphere_THourglass':
        _, at_T0 = sampling.NSphere_THourglass.entry(pts, params['shape_param'], 0, 1)
        assert not at_T0[3] and not at_T0[5]
        keep = pts[at_T0]
        pts = torch.cat((keep, keep[:M - keep.shape[0]]), 0)
        assert int((pts[:, 0] >= 0.5).sum()) >= 1                 # (the widening half, inside the inner ball)
    assert pts.shape == (M, 4)
    return pts


def _reference(points, w, params, theta, P, n_sub):
    """per point, on the CPU: n = max(1, ceil((t - T0) / step)) equal steps ending at t, refspec.u_net on the one-path group with
    start = func_h([T0, x]), autograd in theta: (u [M], {key: sum_p w_p du_p/dtheta[key]})"""
    from oracle import refspec as R
    T0, T = params['T0'], params['T']
    th = {k: v.clone().requires_grad_(True) for k, v in theta.items()}
    keys = list(th)
    total = {k: torch.zeros_like(v) for k, v in theta.items()}
    u = []
    for p, wp in zip(points, w):
        t, x = float(p[0]), p[1:]
        n = 0 if t == T0 else max(1, math.ceil((t - T0) / ((T - T0) / n_sub)))
        grid = torch.tensor([T0 + (t - T0) * k / n for k in range(n)] + [t], dtype=F64)
        X = torch.cat((grid.view(1, -1, 1), x.view(1, 1, -1).expand(1, n + 1, -1)), 2)
        ui = R.u_net(th, params, X, P.func_h(X[:, 0, :]).reshape(-1)).reshape(-1)[-1]
        for k, g in zip(keys, torch.autograd.grad(ui, [th[k] for k in keys], allow_unused=True)):
            if g is not None:
                total[k] += wp * g
        u.append(ui.detach())
    return torch.stack(u), total


def _check_params(S, r, ref, m, what, record=None):
    from oracle import refspec as R
    named = dict(S.u_net.module.named_parameters())
    assert list(r['params']) == list(named)
    for name, key in R.u_names(m):
        name = name[len('module.'):]
        got = r['params'][name]
        assert got.shape == named[name].shape and got.dtype == F64 and got.is_cuda and not got.requires_grad, name
        scale = float(ref[key].abs().max())
        assert scale > 0, name
        err = float((got.cpu() - ref[key].view(got.shape)).abs().max()) / scale
        if record is not None:
            record[key] = max(record.get(key, 0.0), err)
        assert err < TOL_G, '%s %s: max rel-to-scale error %.3e' % (name, what, err)


@pytest.mark.parametrize('domain,funcs,method', [('Hypercube', 'Ex4_1', 'midpoint'), ('NSphere_TCone', 'Ex4_3', 'rk4'),
                                                 ('NSphere_THourglass', 'Ex4_3', 'euler')])
def test_solver_evaluate_vjp_matches_a_per_point_reference(domain, funcs, method):
    import dataclasses
    P = importlib.import_module('configs.%s_funcs' % funcs)
    S, params = _solver(domain, P, 20, 10, 8, method)
    theta = _theta_of(S, 8)
    pts = _entered_at_T0(domain, params)
    w = _weights(M, 31)
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()[1].copy())
    r = S.evaluate_vjp(pts, w)
    assert torch.equal(torch.get_rng_state(), rng[0]) and torch.equal(torch.cuda.get_rng_state(), rng[1])
    assert (np.random.get_state()[1] == rng[2]).all()
    assert set(r) == {'u', 'params', 'start'} and r['u'].shape == (M,) and r['start'].shape == (M,)
    assert torch.equal(r['u'], S.evaluate(pts))                  # the forward's bits
    u_ref, g_ref = _reference(pts, w, params, theta, P, params['N_t'])
    worst = {}
    _close(r['u'], u_ref, TOL_T, 'u ' + domain)
    _check_params(S, r, g_ref, 8, domain, worst)
    print('largest error against the per-point reference, %s %s: %.2e' % (domain, method, max(worst.values())))
    # device points, another resolution, the module's own entry point
    r5 = S.u_net.module.evaluate_vjp(pts.cuda(), w.cuda(), n_sub=5)
    assert torch.equal(r5['u'], S.evaluate(pts.cuda(), n_sub=5))
    _check_params(S, r5, _reference(pts, w, params, theta, P, 5)[1], 8, domain + ' n_sub 5')
    # float32 points and weights are widened exactly
    p32, w32 = pts.float(), w.float()
    r32 = S.evaluate_vjp(p32, w32)
    _check_params(S, r32, _reference(p32.double(), w32.double(), params, theta, P, params['N_t'])[1], 8, domain + ' float32')
    # chunks of 16 paths: u to the bit, the gradient in another order of the slabs' sum
    S.options = dataclasses.replace(S.options, eval_chunk_paths=16)
    r16 = S.evaluate_vjp(pts, w)
    assert torch.equal(r16['u'], r['u']) and torch.equal(r16['start'], r['start'])
    for k in r['params']:
        _close(r16['params'][k], r['params'][k], TOL_T, 'chunks of 16 ' + k)


def test_evaluate_fn_trains_through_autograd():
    import configs.Ex4_1_funcs as P
    S, params = _solver('Hypercube', P, 20, 10, 8, 'midpoint')
    net = S.u_net.module
    pts = _entered_at_T0('Hypercube', params)
    data = torch.randn(M, dtype=F64, generator=torch.Generator().manual_seed(41)).cuda()
    before = S.evaluate_grad(pts)
    plist = list(net.parameters())
    u = net.evaluate_fn(pts)
    assert u.requires_grad and u.shape == (M,) and torch.equal(u.detach(), S.evaluate(pts))
    loss = ((u - data) ** 2).mean()
    grads = torch.autograd.grad(loss, plist)
    # the same cotangent through evaluate_vjp: to the bit
    leaf = u.detach().clone().requires_grad_(True)
    gu, = torch.autograd.grad(((leaf - data) ** 2).mean(), leaf)
    r = net.evaluate_vjp(pts, gu)
    for (name, _), g in zip(net.named_parameters(), grads):
        assert torch.equal(g, r['params'][name]), name
    # ... and the CPU reference
    theta = _theta_of(S, 8)
    _check_params(S, r, _reference(pts, gu.cpu(), params, theta, P, params['N_t'])[1], 8, 'least squares')
    after = S.evaluate_grad(pts)
    for k in before:
        assert torch.equal(after[k], before[k]), 'evaluate_grad moved: ' + k
    # one SGD step: the parameters stay views of the blob, evaluate() sees the new weights
    saved = net.blob.data.clone()
    opt = torch.optim.SGD(net.parameters(), lr=1e-2)
    opt.zero_grad()
    ((net.evaluate_fn(pts) - data) ** 2).mean().backward()
    for p, g in zip(plist, grads):
        assert torch.equal(p.grad, g)
    opt.step()
    net.blob.check_alias()
    assert not torch.equal(net.blob.data, saved)
    stepped = S.evaluate(pts)
    assert not torch.equal(stepped, u.detach())
    _close(stepped, _reference(pts, gu.cpu(), params, _theta_of(S, 8), P, params['N_t'])[0], TOL_T, 'evaluate after the step')
    with torch.no_grad():
        net.blob.data.copy_(saved)
    net.blob.check_alias()
    again = S.evaluate_grad(pts)
    for k in before:
        assert torch.equal(again[k], before[k]), 'evaluate_grad after the step sequence: ' + k


def test_surface_refusals():
    import configs.Ex4_1_funcs as P1
    import configs.Ex4_3_funcs as P3
    from xnode_wan_pde_solver_amd._lib import XnwanError
    pts = _eval_points('Hypercube')
    w = _weights(M, 5)
    for name in ('dopri5', 'explicit_adams'):
        S, _ = _solver('Hypercube', P1, 20, 10, 8, name)
        with pytest.raises(XnwanError, match=r'evaluate_vjp\(\).*' + name + '.*fixed-grid'):
            S.evaluate_vjp(pts, w)
        with pytest.raises(XnwanError, match=r'evaluate_vjp\(\).*' + name):
            S.u_net.module.evaluate_fn(pts)
    S, _ = _solver('Hypercube', P1, 20, 10, 8, 'midpoint')
    with pytest.raises(XnwanError, match=r'w must be a tensor \[M\] = \[37\]'):
        S.evaluate_vjp(pts, w.view(M, 1))
    with pytest.raises(XnwanError, match=r'evaluate_fn\(\): points that require grad.*evaluate_grad\(\)'):
        S.u_net.module.evaluate_fn(pts.clone().requires_grad_(True))
    S, _ = _solver('NSphere_THourglass', P3, 20, 10, 8, 'euler')
    from xnode_wan_pde_solver_amd import sampling
    hg = _eval_points('NSphere_THourglass')
    _, at_T0 = sampling.NSphere_THourglass.entry(hg, 1.0, 0, 1)
    first = int((~at_T0).nonzero()[0])
    assert not at_T0[3] and first <= 3
    with pytest.raises(XnwanError, match='entered at T0') as e:
        S.evaluate_vjp(hg, w)
    assert '%d points' % int((~at_T0).sum()) in str(e.value) and 'point %d' % first in str(e.value)
    assert S.evaluate(hg).shape == (M,)      # (evaluate() serves them, as before)
