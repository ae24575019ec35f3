"""The gradient at scattered points with solver 'dopri5' on the device: the per-path forward with its checkpoints kept (csrc/xw_tdopri_paths.hip
through xw_paths_dopri5_ckpt_fwd), the reverse sweep over every path's own record (csrc/xw_tdopri_paths_grad.hip: kq_paths_grad,
kernels.paths_dopri5_grad) and the chain built on them (evalpaths.evaluate_points_grad, XNODE.evaluate_grad, NODE_WAN_solver.evaluate_grad).

Kernel level, inside the guard-banded, poisoned arena of tests/guarded.py, on the fixtures of tests/test_gpu_eval_dopri5.py (every tile
holds a whole-interval path, a path with t_end == t_in and a 100x start value; the seeds meet the gap and condition premises that file
asserts -- the forward is the same kernel).  The specification of every path is tests/dopri5_ref.py::dopri5 on that path ALONE, frozen
on the path's own recorded steps, with the sample times [t_in, the starts of its steps 1 .. n_acc - 1, t_end]: one solve gives the state
at the start of every step (ckpt: 1e-9 relative to the path's largest entry, that file's bound for Y, and its reasoning), y(t_end) for
ut = FL_w . field(t_end, x, y(t_end)) (1e-9, Y's bound) and, under autograd in x and start, gx and gs (1e-9 relative to scale, the bound
tests/test_gpu_dopri5_tiled.py::test_sweep_against_frozen_grid_autograd holds kq_sweep to, with the same arithmetic; the paths whose
start value is 100x the others' are a scale of their own, as u is in test_gpu_eval_dopri5.py).  The value at t_end comes from the last
step's dense output whatever other sample times the solve has, so it is the solve with [t_in, t_end].
Poison: slots of rec and ckpt at or past a path's n_acc hold the arena's NaN pattern when the sweep reads the record -- an idle lane that
took t0, dt or its state from them would turn its outputs NaN.  Bitwise: with and without ckpt in the forward; under a permutation of the
paths; every output alone; a larger cap; a captured-graph replay; every path on one grid against the N = 1 launch.
Public surface: evaluate_grad with solver 'dopri5' on the cube and the hourglass's T0-entered points (the tanh-only networks, where
test_gpu_eval_dopri5.py holds u to 1e-9 against the free-running restatement) against a per-point CPU loop: dopri5_ref free on the
point, then frozen on the steps it took, under autograd through x and through h([T0, x])."""
import dataclasses
import importlib
import os
import sys
from unittest import mock

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dopri5_ref as D  # noqa: E402
import guarded as G  # noqa: E402
import test_gpu_eval_dopri5 as E  # noqa: E402
from test_gpu_eval_dopri5 import CAP, NETS, NS, SEEDS, _paths  # noqa: E402
from test_gpu_tiled_stepper import F64, _theta  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-9
I32, I64 = torch.int32, torch.int64
OUTS = ('gx', 'gs', 'ut')
FWD_OUTS = ('u', 'Y', 'fin', 'status', 'n_acc', 'n_att')


def _forward(KN, arena, blob, x, start, t_in, t_end, H, K, m, cap=CAP, ckpt=True):
    """one guarded launch of the per-path forward with u, Y, rec, fin and (ckpt) the checkpoints: the job"""
    N = x.shape[0]
    ints = {k: arena.out((N + 1) // 2, name=k).view(I32) for k in ('status', 'n_acc', 'n_att')}
    job = dict(xT=arena.inp(x.t(), name='xT'), start=arena.inp(start, name='start'), t_in=arena.inp(t_in, name='t_in'),
               t_end=arena.inp(t_end, name='t_end'), u=arena.out(N, name='u'), Y=arena.out(H, N, name='Y'),
               rec=arena.out(cap, 2, N, name='rec'), fin=arena.out(2, N, name='fin'), ints=ints, **{k: v[:N] for k, v in ints.items()})
    if ckpt:
        job['ckpt'] = arena.out(cap, H, N, name='ckpt')
    KN.paths_dopri5_fwd([job], blob, H, K, m, H)
    return job


def _sweep(KN, arena, blob, fj, H, K, m, want=OUTS):
    """one guarded launch of the sweep on the forward job fj: the job with the outputs asked for"""
    d, N = fj['xT'].shape
    job = {k: fj[k] for k in ('xT', 'start', 't_in', 't_end', 'n_acc', 'rec', 'ckpt', 'Y')}
    for k in want:
        job[k] = arena.out(*((d, N) if k == 'gx' else (N,)), name=k)
    KN.paths_dopri5_grad([job], blob, H, K, m)
    return job


def _check_forwards(arena, jobs, written=()):
    """every output element of the forward jobs written, rec below n_acc and ckpt below max(n_acc, 1) and nothing else of them, no
    guard element touched -- the workspaces' included; `written`: further outputs, every element of them"""
    E._check_written(arena, jobs)                                # (u, Y, fin, rec, the int32 words)
    written, untouched = list(written), []
    for j in jobs:
        if 'ckpt' in j:
            cap, H, N = j['ckpt'].shape
            mask = (torch.arange(cap, device=j['ckpt'].device).view(cap, 1, 1) < j['n_acc'].clamp(min=1).view(1, 1, N)).expand(cap, H, N)
            written.append((j['ckpt'], mask))
            untouched.append((j['ckpt'], ~mask))
    arena.check(written=written, untouched=untouched)


_REF = {}


def _ref(net, i, steps):
    """path i of the net's case on its recorded steps, alone: dict(slots [n, H] -- the state at the start of every step, slot 0 the
    lifted start value --, gx [d], gs, ut), once per distinct record"""
    key = (net, i, tuple(steps))
    if key not in _REF:
        from oracle import refspec as R
        d, H, K, m = NETS[net]
        theta, _ = _theta(H, K, m, d, 500 + net)
        th = {k: v.detach() for k, v in theta.items()}
        x, start, t_in, t_end, _ = _paths(d, SEEDS[net])
        xi = x[i].view(1, -1).clone().requires_grad_(True)
        si = start[i].view(1, 1).clone().requires_grad_(True)
        y0 = torch.relu(torch.relu(si @ th['IL0_w'].T + th['IL0_b']) @ th['IL2_w'].T + th['IL2_b']) @ th['IL4_w'].T + th['IL4_b']
        times = torch.stack([t_in[i]] + [torch.tensor(a, dtype=F64) for a, _ in steps[1:]] + [t_end[i]])
        ys, _ = D.dopri5(lambda t, y: R.field(th, m, xi, t, y), y0, times, count=y0.numel(), frozen=list(steps))
        y_end = ys[0, -1]
        u = y_end @ th['FL_w'].reshape(-1) + th['FL_b'].reshape(())
        gx, gs = torch.autograd.grad(u, [xi, si], allow_unused=True)
        ut = (R.field(th, m, xi.detach(), t_end[i], y_end.detach().view(1, -1)) @ th['FL_w'].T).reshape(())
        _REF[key] = dict(slots=ys[0, :-1].detach(), gx=torch.zeros(d, dtype=F64) if gx is None else gx.reshape(-1), gs=gs.reshape(()),
                         ut=ut, u=float(u.detach()))
    return _REF[key]


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('net', range(len(NETS)))
def test_forward_keeps_the_state_at_the_start_of_every_accepted_step(net, N):
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m = NETS[net]
    _, blob_h = _theta(H, K, m, d, 500 + net)
    x, start, t_in, t_end, _ = (a[:N] for a in _paths(d, SEEDS[net]))
    arena = G.Arena(torch.device('cuda'))
    with arena.workspaces(KN):
        blob = arena.inp(blob_h, name='theta')
        plain = _forward(KN, arena, blob, x, start, t_in, t_end, H, K, m, ckpt=False)
        kept = _forward(KN, arena, blob, x, start, t_in, t_end, H, K, m)
        short = _forward(KN, arena, blob, x, start, t_in, t_end, H, K, m, cap=2)
    _check_forwards(arena, (plain, kept, short))
    what = 'net %s N %d' % (NETS[net], N)
    assert not bool(kept['status'].any()) and int(kept['n_acc'].max()) < CAP, what
    # the same bits with and without the checkpoints (rec as bit patterns: unwritten slots hold the poison in both)
    for k in FWD_OUTS:
        assert torch.equal(kept[k], plain[k]) and torch.equal(short[k], plain[k]), k + ' ' + what
    assert torch.equal(kept['rec'].view(I64), plain['rec'].view(I64)), what
    two = (torch.arange(2, device=kept['n_acc'].device).view(2, 1, 1) < kept['n_acc'].clamp(min=1).view(1, 1, N)).expand(2, H, N)
    assert torch.equal(short['ckpt'][two], kept['ckpt'][:2][two]), 'short record ' + what
    # slot s of path p against the restatement on that path alone, frozen on its own steps
    ck, worst = kept['ckpt'].cpu(), 0.0
    for i in range(N):
        steps = E._steps_of(kept, i)
        want = _ref(net, i, steps)['slots']
        assert want.shape == (max(len(steps), 1), H)
        for s in range(want.shape[0]):
            worst = max(worst, E._rel(ck[s, :, i], want[s]))
    print('%s: accepted %d..%d; worst checkpoint %.2e' % (what, int(kept['n_acc'].min()), int(kept['n_acc'].max()), worst))
    assert worst < TOL, what


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('net', range(len(NETS)))
def test_sweep_over_every_paths_own_record(net, N):
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m = NETS[net]
    _, blob_h = _theta(H, K, m, d, 500 + net)
    x, start, t_in, t_end, big = (a[:N] for a in _paths(d, SEEDS[net]))
    dev = torch.device('cuda')
    arena = G.Arena(dev)
    with arena.workspaces(KN):
        blob = arena.inp(blob_h, name='theta')
        fj = _forward(KN, arena, blob, x, start, t_in, t_end, H, K, m)
        torch.cuda.synchronize()
        kept = {k: fj[k].clone() for k in ('xT', 'start', 't_in', 't_end', 'n_acc', 'rec', 'ckpt', 'Y')}
        kept['theta'] = blob.clone()
        full = _sweep(KN, arena, blob, fj, H, K, m)
        alone = {k: _sweep(KN, arena, blob, fj, H, K, m, want=(k,)) for k in OUTS}
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(100 * net + N + 1))
        fm = _forward(KN, arena, blob, x[perm], start[perm], t_in[perm], t_end[perm], H, K, m)
        moved = _sweep(KN, arena, blob, fm, H, K, m)
        fw = _forward(KN, arena, blob, x, start, t_in, t_end, H, K, m, cap=CAP + 7)
        wide = _sweep(KN, arena, blob, fw, H, K, m)
        # every path on the grid of path 0 (the whole interval): each column is the N = 1 launch
        one = lambda a: a[:1].expand(N, *a.shape[1:]).contiguous()                      # noqa: E731
        fs = _forward(KN, arena, blob, one(x), one(start), one(t_in), one(t_end), H, K, m)
        shared = _sweep(KN, arena, blob, fs, H, K, m)
        f1 = _forward(KN, arena, blob, x[:1], start[:1], t_in[:1], t_end[:1], H, K, m)
        single = _sweep(KN, arena, blob, f1, H, K, m)
    # every output element written (so: none of them NaN), no guard element touched -- the workspaces' included
    sweeps = [full, moved, wide, shared, single] + list(alone.values())
    _check_forwards(arena, (fj, fm, fw, fs, f1), written=[j[k] for j in sweeps for k in OUTS if k in j])
    what = 'net %s N %d' % (NETS[net], N)
    # the record, the checkpoints (their poisoned slots too), the inputs and theta hold the bits they held
    for k in ('xT', 'start', 't_in', 't_end', 'rec', 'ckpt', 'Y'):
        assert torch.equal(fj[k].view(I64), kept[k].view(I64)), '%s changed: %s' % (k, what)
    assert torch.equal(fj['n_acc'], kept['n_acc']) and torch.equal(blob, kept['theta']), what
    n_acc = fj['n_acc'].cpu()
    assert not bool(fj['status'].any()) and int(n_acc.max()) < CAP, what
    if N > 2:                                                        # no step beside many, and the large start's own count, in one tile
        assert int(n_acc[1]) == 0 and len({int(n_acc[0]), int(n_acc[1]), int(n_acc[2])}) == 3, what
    # the same bits: each output alone, beside other neighbours, with a larger cap, on a shared grid
    pd = perm.to(dev)
    for k in OUTS:
        assert torch.equal(alone[k][k], full[k]), 'alone %s %s' % (k, what)
        assert torch.equal(moved[k], full[k][..., pd]), 'permuted %s %s' % (k, what)
        assert torch.equal(wide[k], full[k]), 'larger cap %s %s' % (k, what)
        assert torch.equal(shared[k], single[k].expand_as(shared[k])), 'shared grid %s %s' % (k, what)
        assert torch.equal(single[k][..., 0], full[k][..., 0]), 'first path alone %s %s' % (k, what)
    for k in FWD_OUTS:
        assert torch.equal(fm[k], fj[k][..., pd]) and torch.equal(fw[k], fj[k]), k + ' ' + what
    # every path against the restatement on that path alone, frozen on its own record, under autograd
    refs = [_ref(net, i, E._steps_of(fj, i)) for i in range(N)]
    gx_r, gs_r = torch.stack([r['gx'] for r in refs], 1), torch.stack([r['gs'] for r in refs])
    ut_r = torch.stack([r['ut'] for r in refs])
    worst = dict(gx=0.0, gs=0.0, ut=0.0)
    for grp in (big, ~big):
        if bool(grp.any()):
            worst['gx'] = max(worst['gx'], E._rel(full['gx'].cpu()[:, grp], gx_r[:, grp]))
            worst['gs'] = max(worst['gs'], E._rel(full['gs'].cpu()[grp], gs_r[grp]))
            worst['ut'] = max(worst['ut'], E._rel(full['ut'].cpu()[grp], ut_r[grp]))
    print('%s: accepted %d..%d; worst gx %.2e gs %.2e ut %.2e (scales %.2e %.2e %.2e)'
          % (what, int(n_acc.min()), int(n_acc.max()), worst['gx'], worst['gs'], worst['ut'], float(gx_r.abs().max()),
             float(gs_r.abs().max()), float(ut_r.abs().max())))
    assert float(gx_r.abs().max()) > 0 and float(gs_r.abs().max()) > 0 and float(ut_r.abs().max()) > 0     # (not a comparison of zeros)
    assert worst['gx'] < TOL and worst['gs'] < TOL and worst['ut'] < TOL, what
    nostep = (n_acc == 0).to(dev)
    assert bool((full['gx'][:, nostep] == 0).all()), 'a path without a step has no x gradient: ' + what


def test_graph_replay_gives_the_same_bits():
    from xnode_wan_pde_solver_amd import kernels as KN
    net, N = 3, E.NMAX
    d, H, K, m = NETS[net]
    _, blob_h = _theta(H, K, m, d, 500 + net)
    x, start, t_in, t_end, _ = _paths(d, SEEDS[net])
    dev = torch.device('cuda')
    z = lambda *s: torch.empty(*s, dtype=F64, device=dev)                               # noqa: E731
    job = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), t_in=t_in.to(dev), t_end=t_end.to(dev), u=z(N), Y=z(H, N),
               rec=z(CAP, 2, N), ckpt=z(CAP, H, N), status=torch.empty(N, dtype=I32, device=dev),
               n_acc=torch.empty(N, dtype=I32, device=dev), n_att=torch.empty(N, dtype=I32, device=dev))
    outs = dict(gx=z(d, N), gs=z(N), ut=z(N))
    blob = blob_h.to(dev)
    job['rec'].fill_(float('nan'))
    job['ckpt'].fill_(float('nan'))
    KN.paths_dopri5_fwd([job], blob, H, K, m, H)
    KN.paths_dopri5_grad([dict(job, **outs)], blob, H, K, m)
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in outs.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        KN.paths_dopri5_grad([dict(job, **outs)], blob, H, K, m)   # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for v in outs.values():
        v.fill_(float('nan'))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        KN.paths_dopri5_grad([dict(job, **outs)], blob, H, K, m)
    g.replay()
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert torch.equal(v, first[k]) and not bool(torch.isnan(v).any()), k


def test_wrapper_refusals():
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    d, H, K, m = NETS[0]
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 1)
    bc = blob.to(dev)
    z = lambda *s: torch.zeros(*s, dtype=F64, device=dev)                               # noqa: E731
    i = torch.zeros(5, dtype=I32, device=dev)
    job = dict(xT=z(d, 5), start=z(5), t_in=z(5), t_end=z(5), n_acc=i, rec=z(3, 2, 5), ckpt=z(3, H, 5), Y=z(H, 5), gs=z(5))
    for k in ('n_acc', 'rec', 'ckpt'):
        with pytest.raises(XnwanError, match=k + ', as paths_dopri5_fwd wrote it'):
            KN.paths_dopri5_grad([{a: b for a, b in job.items() if a != k}], bc, H, K, m)
    with pytest.raises(XnwanError, match='n_acc must be'):
        KN.paths_dopri5_grad([dict(job, n_acc=z(5))], bc, H, K, m)
    with pytest.raises(XnwanError, match='ckpt must have shape'):
        KN.paths_dopri5_grad([dict(job, ckpt=z(4, H, 5))], bc, H, K, m)                # (another cap than rec's)
    with pytest.raises(XnwanError, match='rec must have shape'):
        KN.paths_dopri5_grad([dict(job, rec=z(0, 2, 5), ckpt=z(0, H, 5))], bc, H, K, m)
    with pytest.raises(XnwanError, match='no output'):
        KN.paths_dopri5_grad([{a: b for a, b in job.items() if a != 'gs'}], bc, H, K, m)
    with pytest.raises(XnwanError, match='ut needs Y'):
        KN.paths_dopri5_grad([dict({a: b for a, b in job.items() if a != 'Y'}, ut=z(5))], bc, H, K, m)
    fwd = dict(xT=z(d, 5), start=z(5), t_in=z(5), t_end=z(5), u=z(5), status=i.clone(), n_acc=i.clone(), n_att=i.clone())
    with pytest.raises(XnwanError, match="ckpt must have shape .* = rec's 3"):
        KN.paths_dopri5_fwd([dict(fwd, rec=z(3, 2, 5), ckpt=z(4, H, 5))], bc, H, K, m, H)
    with pytest.raises(XnwanError, match='ckpt must have shape'):
        KN.paths_dopri5_fwd([dict(fwd, ckpt=z(0, H, 5))], bc, H, K, m, H)
    with pytest.raises(XnwanError, match='ckpt must have shape'):
        KN.paths_dopri5_fwd([dict(fwd, ckpt=z(2, H + 1, 5))], bc, H, K, m, H)


# ---- the public surface ----------------------------------------------------------------------------------------------------------------
SURFACE = [s for s in E.SURFACE if s[4] == 1]                    # the tanh-only networks
M_POINTS = E.M_POINTS


def _reference(points, params, theta, P):
    """per point entered at T0, on the CPU: dopri5_ref free on the one-path group [[T0, x], [t, x]], then frozen on the steps it took,
    under autograd through x on both ways -- the field's input and the start value h([T0, x]); ut from refspec.field at (t, x, y(t)):
    (u, grad, ut, min gap)"""
    from oracle import refspec as R
    T0, m = float(params['T0']), params['u_layers']
    u, grad, ut, gap = [], [], [], float('inf')
    for p in points:
        t = p[0]
        x = p[1:].clone().requires_grad_(True)
        X = torch.cat((torch.stack((torch.tensor(T0, dtype=F64), t)).view(1, 2, 1), x.view(1, 1, -1).expand(1, 2, -1)), 2)
        s = P.func_h(X[:, 0, :]).reshape(-1)
        with torch.no_grad():
            u_free, info = D.u_net(theta, params, X, s)
        gap = min(gap, info['gap'])
        sv = s.reshape(-1, 1).to(F64)
        y0 = torch.relu(torch.relu(sv @ theta['IL0_w'].T + theta['IL0_b']) @ theta['IL2_w'].T + theta['IL2_b']) @ theta['IL4_w'].T + theta['IL4_b']
        xi = x.view(1, -1)
        ys, _ = D.dopri5(lambda tt, y: R.field(theta, m, xi, tt, y), y0, X[0, :, 0].detach(), count=y0.numel(), frozen=info['steps'])
        ui = (ys[0, 1] @ theta['FL_w'].reshape(-1) + theta['FL_b'].reshape(()))
        assert abs(float(ui.detach() - u_free.reshape(-1)[-1])) <= 1e-13 * max(1.0, abs(float(ui.detach())))   # (the same solve)
        gi, = torch.autograd.grad(ui, x, allow_unused=True)
        u.append(ui.detach())
        grad.append(torch.zeros_like(x) if gi is None else gi)
        ut.append((R.field(theta, m, xi.detach(), t, ys[:, 1].detach()) @ theta['FL_w'].T).reshape(()))
    return torch.stack(u), torch.stack(grad), torch.stack(ut), gap


@pytest.mark.parametrize('domain,funcs,H,K,m', SURFACE)
def test_evaluate_grad_with_dopri5_matches_a_per_point_reference(domain, funcs, H, K, m):
    from test_gpu_eval_paths import _eval_points, _theta_of
    from xnode_wan_pde_solver_amd import evalpaths as EP, sampling
    P = importlib.import_module('configs.%s_funcs' % funcs)
    pts = _eval_points(domain, M=M_POINTS)
    if domain == 'Hypercube':
        S, params = E._dopri5_solver(domain, P, H, K, m)
        evaluate, evaluate_grad, module, theta = S.evaluate, S.evaluate_grad, S.u_net.module, _theta_of(S, m)
    else:                                                        # (XNODE directly: E._surface says why)
        evaluate, module, params, theta = E._surface(domain, P, H, K, m)
        evaluate_grad = module.evaluate_grad
        _, at_T0 = sampling.NSphere_THourglass.entry(pts, params['shape_param'], 0, 1)
        assert 5 < int(at_T0.sum()) < M_POINTS
        pts = pts[at_T0].contiguous()                            # the T0-entered points: both halves of the hourglass
        assert int((pts[:, 0] > 0.5).sum()) > 2
    M, d = pts.shape[0], pts.shape[1] - 1
    passes = []
    inner = EP.dopri5_grad_pass

    def spy(*a, **kw):
        passes.append(inner(*a, **kw))
        return passes[-1]
    with mock.patch.object(EP, 'dopri5_grad_pass', spy):
        r = evaluate_grad(pts)                                   # host points, float64
    assert set(r) == {'u', 'grad', 'ut'}
    assert r['u'].shape == (M,) and r['grad'].shape == (M, d) and r['ut'].shape == (M,)
    assert all(v.dtype == F64 and v.is_cuda and not v.requires_grad for v in r.values())
    # u: the bits of evaluate(); the second forward's u, in the first pass's order, is that as well
    assert torch.equal(r['u'], evaluate(pts))
    third, = passes
    _, inverse = EP.sort_by_steps(pts[:, 0] - params['T0'])      # (the first pass's sort: by the length of the interval)
    assert torch.equal(third['u'][inverse.cuda()], r['u'])
    u_r, grad_r, ut_r, gap = _reference(pts, params, theta, P)
    err = dict(u=E._rel(r['u'], u_r), grad=E._rel(r['grad'], grad_r), ut=E._rel(r['ut'], ut_r))
    print('evaluate_grad %s (%d, %d, %d): rel-to-scale errors %s, min gap %.2e' % (domain, H, K, m, err, gap))
    assert gap > 1e-9, 'bad fixture: a step decision within %.1e of the threshold' % gap
    assert float(grad_r.abs().max()) > 0 and float(ut_r.abs().max()) > 0
    assert err['u'] < TOL and err['grad'] < TOL and err['ut'] < TOL
    # chunks of 16 paths: the same bits
    r16 = module.evaluate_grad(pts, chunk=16)
    for k in r:
        assert torch.equal(r16[k], r[k]), k
    if domain == 'Hypercube':                                    # ... through the option as well
        S.options = dataclasses.replace(S.options, eval_chunk_paths=16)
        r16 = S.evaluate_grad(pts)
        for k in r:
            assert torch.equal(r16[k], r[k]), k
    # float32 points are widened exactly; device points: h and its gradient are then evaluated on the device (their last bits may differ)
    p32 = pts.float()
    a, b = evaluate_grad(p32), evaluate_grad(p32.double())
    for k in a:
        assert torch.equal(a[k], b[k]), k
    rd = module.evaluate_grad(pts.cuda())
    assert E._rel(rd['u'], u_r) < TOL and E._rel(rd['grad'], grad_r) < TOL and E._rel(rd['ut'], ut_r) < TOL


def test_evaluate_grad_names_the_first_point_at_the_step_limit():
    import configs.Ex4_1_funcs as P
    from test_gpu_eval_paths import _eval_points
    from xnode_wan_pde_solver_amd._lib import XnwanError
    S, params = E._dopri5_solver('Hypercube', P, 20, 10, 8)
    pts = _eval_points('Hypercube', M=M_POINTS)
    pts[0, 0] = 0.0                                              # t == t_in: no step, never at the limit
    with pytest.raises(XnwanError, match='step limit of 1 accepted steps') as e:
        S.u_net.module.evaluate(pts, max_steps=1)
    named = str(e.value)[len('evaluate(): '):]
    assert 'first: point ' in named and 'first: point 0,' not in named
    S.options = dataclasses.replace(S.options, dopri5_max_steps=1)
    with pytest.raises(XnwanError, match='step limit of 1 accepted steps') as e:
        S.evaluate_grad(pts)
    assert str(e.value) == 'evaluate_grad(): ' + named         # the same count, the same point, the same controller state
    net = S.u_net.module
    net.dopri5_max_steps = 1                                     # ... and the module's own limit
    with pytest.raises(XnwanError, match='step limit of 1 accepted steps') as e:
        net.evaluate_grad(pts)
    assert str(e.value) == 'evaluate_grad(): ' + named
    with pytest.raises(XnwanError, match="n_sub = 3 with solver 'dopri5'"):
        S.evaluate_grad(pts, n_sub=3)


def test_midpoint_evaluate_grad_returns_the_bits_of_the_per_path_kernels():
    """evaluate_grad with a fixed-grid solver is what it was: evalpaths' grids on kernels.tiled_paths_fwd / tiled_paths_grad, directly"""
    import configs.Ex4_1_funcs as P
    from test_gpu_eval_paths import _eval_points, _solver
    from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN
    S, params = _solver('Hypercube', P, 20, 10, 8, 'midpoint')
    pts = _eval_points('Hypercube', M=M_POINTS)
    r = S.evaluate_grad(pts)
    net = S.u_net.module
    dev = net.blob.data.device
    H, K = net.kdims
    t, t_in = pts[:, 0].contiguous(), torch.zeros(M_POINTS, dtype=F64)
    first = torch.cat((t_in.view(-1, 1), pts[:, 1:]), 1)
    s = P.func_h(first).reshape(-1).double()
    n = EP.step_counts(t, t_in, 0, 1, params['N_t'])
    order, inverse = EP.sort_by_steps(n)
    tT = EP.pack_grids(t[order], t_in[order], n[order]).to(dev)
    L = tT.shape[0]
    job = dict(xT=pts[order, 1:].t().contiguous().to(dev), start=s[order].contiguous().to(dev), tT=tT, nstep=n[order].to(I32).to(dev),
               u=torch.empty(L, M_POINTS, dtype=F64, device=dev), Y=torch.empty(L, H, M_POINTS, dtype=F64, device=dev),
               gx=torch.empty(3, M_POINTS, dtype=F64, device=dev), gs=torch.empty(M_POINTS, dtype=F64, device=dev),
               ut=torch.empty(M_POINTS, dtype=F64, device=dev))
    mid = KN.METHODS['midpoint']
    KN.tiled_paths_fwd([job], net.blob.data, mid, H, K, 8)
    KN.tiled_paths_grad([job], net.blob.data, mid, H, K, 8)
    inv = inverse.to(dev)
    assert torch.equal(r['u'], job['u'][L - 1][inv]) and torch.equal(r['ut'], job['ut'][inv])
    hx = EP.start_gradient(P.func_h, first).to(dev)
    assert torch.equal(r['grad'], job['gx'].t()[inv] + job['gs'][inv].view(-1, 1) * hx)
