"""Solver 'dopri5' with a step controller per path (csrc/xw_tdopri_paths.hip: kq_paths) and the evaluation at scattered points built
on it (kernels.paths_dopri5_fwd, evalpaths.paths_dopri5, XNODE.evaluate / NODE_WAN_solver.evaluate) on the device.

Kernel level, inside the guard-banded, poisoned arena of tests/guarded.py.  Every path is compared with tests/dopri5_ref.py::dopri5
run on that path ALONE with the sample times [t_in, t_end] -- the specification.  The bounds and their reasoning are those of
tests/test_gpu_dopri5.py for its one-path cases: on tanh-only fields the step decisions are pinned exactly (fixtures with
gap = min |ratio - 1| > 1e-9, asserted) and the grids agree to GRID_TOL = 1e-9, u and Y to 1e-9; with ReLU layers in the field the
decisions are not a smooth function of the rounding, so u and Y are compared at 1e-9 with the restatement on the path's own recorded
steps, and at 1e-4 with the free-running one.  Y is compared path by path, relative to the path's largest entry; u, one number per
path, relative to the largest |u| among the paths of its start scale (the paths whose start value is 100x the others' apart).
Bitwise: a permutation of the paths, a captured-graph replay, chunks of 16, with and without Y / rec / fin, a short rec.  Every output
element written, no guard element touched (the workspace's included).  Limits: max_steps and max_attempts give XW_DOPRI_STEPS to exactly
the paths that need more, their tile neighbours keep their bits.
Public surface: evaluate with solver 'dopri5' on the cube and the hourglass against a per-point CPU loop over dopri5_ref.u_net with the
same callables; float32 and host points; the error that names the first point at the step limit; midpoint evaluate unchanged."""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dopri5_ref as D  # noqa: E402
import guarded as G  # noqa: E402
from test_gpu_tiled_stepper import F64, _theta  # noqa: E402

pytestmark = pytest.mark.gpu

GRID_TOL = 1e-9
TOL, TOL_FREE = 1e-9, 1e-4
# The premise of GRID_TOL, as a fixture check beside the gap.  dopri5_ref.dopri5 reports, per attempt, the condition number of the
# error ratio -- the estimate is a sum of seven terms that nearly cancel -- and whether the next step size moves with it: one unit of
# relative rounding in the terms moves the ratio by `cond` units and the next step size by cond / 5.  The device's terms differ from
# the restatement's by a couple of units of 1.1e-16 (fma chains, the last bits of its tanh): with cond <= 2e7 that is at most
# 2 x 1.1e-16 x 2e7 / 5 = 8.8e-10 < GRID_TOL.  A field that a large start value saturates cancels far deeper (cond 1e8 .. 1e10 was seen
# for most seeds' 100x paths, from the restatement alone), and two correct implementations then differ by more than GRID_TOL: the
# seeds below are chosen on the CPU so that every path, the 100x ones included, meets the premise.
COND_MAX = 2e7
NETS = ((3, 20, 10, 1), (20, 65, 16, 1), (3, 20, 10, 8), (5, 96, 32, 8))      # (d, H, K, m): two tanh-only fields, two with ReLU layers
SEEDS = (280, 45, 13, 14)
NS = (1, 15, 16, 17, 37)
NMAX, CAP = 37, 96
STEPS = 2                                                                     # XW_DOPRI_STEPS (include/xnwan.h)
I32 = torch.int32
POISON_LO, POISON_HI = G.PATTERN & 0xFFFFFFFF, G.PATTERN >> 32                # the two int32 halves of a poisoned double


def _paths(d, seed):
    """NMAX paths, the first N of them a case: x [N, d], start, t_in, t_end.  In every tile of 16, path 0 runs over the whole
    interval [0, 1], path 1 has t_end == t_in (no step) and path 2 a start value 100x the others' (other step counts)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(NMAX, d, generator=g) * 2 - 1).double()
    start = torch.randn(NMAX, dtype=F64, generator=g)
    t_in = 0.5 * torch.rand(NMAX, generator=g, dtype=F64)
    t_end = t_in + 0.05 + 0.45 * torch.rand(NMAX, generator=g, dtype=F64)
    big = torch.zeros(NMAX, dtype=torch.bool)
    for b in range(0, NMAX, 16):
        t_in[b], t_end[b] = 0.0, 1.0
        if b + 1 < NMAX:
            t_end[b + 1] = t_in[b + 1]
        if b + 2 < NMAX:
            start[b + 2] *= 100.0
            big[b + 2] = True
    return x, start, t_in, t_end, big


def _solve(theta, m, x, start, t_in, t_end, frozen=None):
    """the restatement on one path alone: (y(t_end) [H], u, info)"""
    from oracle import refspec as R
    th = {k: v.detach() for k, v in theta.items()}
    s = start.view(1, 1)
    y0 = torch.relu(torch.relu(s @ th['IL0_w'].T + th['IL0_b']) @ th['IL2_w'].T + th['IL2_b']) @ th['IL4_w'].T + th['IL4_b']
    xi = x.view(1, -1)
    ys, info = D.dopri5(lambda t, y: R.field(th, m, xi, t, y), y0, torch.stack((t_in, t_end)), count=y0.numel(), frozen=frozen)
    y = ys[0, 1]
    return y, float(y @ th['FL_w'].reshape(-1) + th['FL_b'].reshape(())), info


_FREE, _FROZEN = {}, {}


def _free(net):
    """the free-running restatement of every path of the net's case, computed once and shared"""
    if net not in _FREE:
        d, H, K, m = NETS[net]
        theta, _ = _theta(H, K, m, d, 500 + net)
        x, start, t_in, t_end, _ = _paths(d, SEEDS[net])
        _FREE[net] = [_solve(theta, m, x[i], start[i], t_in[i], t_end[i]) for i in range(NMAX)]
    return _FREE[net]


def _frozen(net, i, steps):
    """the restatement of path i on the accepted steps `steps`, once per distinct record"""
    key = (net, i, tuple(steps))
    if key not in _FROZEN:
        d, H, K, m = NETS[net]
        theta, _ = _theta(H, K, m, d, 500 + net)
        x, start, t_in, t_end, _ = _paths(d, SEEDS[net])
        _FROZEN[key] = _solve(theta, m, x[i], start[i], t_in[i], t_end[i], frozen=list(steps))
    return _FROZEN[key]


def _launch(KN, arena, blob, x, start, t_in, t_end, H, K, m, want_Y=True, cap=CAP, want_fin=True, **kw):
    N = x.shape[0]
    # the int32 outputs: guarded, poisoned views of ceil(N / 2) doubles of the arena (kept whole under 'ints' for the checks)
    ints = {k: arena.out((N + 1) // 2, name=k).view(I32) for k in ('status', 'n_acc', 'n_att')}
    job = dict(xT=arena.inp(x.t(), name='xT'), start=arena.inp(start, name='start'), t_in=arena.inp(t_in, name='t_in'),
               t_end=arena.inp(t_end, name='t_end'), u=arena.out(N, name='u'), ints=ints, **{k: v[:N] for k, v in ints.items()})
    if want_Y:
        job['Y'] = arena.out(H, N, name='Y')
    if cap:
        job['rec'] = arena.out(cap, 2, N, name='rec')
    if want_fin:
        job['fin'] = arena.out(2, N, name='fin')
    KN.paths_dopri5_fwd([job], blob, H, K, m, H, **kw)
    return job


def _check_written(arena, jobs):
    """every output element written, no guard element touched; rec: the accepted steps below its cap, nothing else"""
    written, untouched = [], []
    for j in jobs:
        written += [j[k] for k in ('u', 'Y', 'fin') if k in j]
        if 'rec' in j:
            cap, _, N = j['rec'].shape
            mask = (torch.arange(cap, device=j['rec'].device).view(cap, 1, 1) < j['n_acc'].view(1, 1, N)).expand(cap, 2, N)
            written.append((j['rec'], mask))
            untouched.append((j['rec'], ~mask))
    arena.check(written=written, untouched=untouched)
    assert min(POISON_LO, POISON_HI) > 1 << 20
    for j in jobs:
        for k, w in j['ints'].items():                          # every word a small count or status, not a poisoned half ...
            N = j[k].numel()
            assert bool((w[:N] >= 0).all()) and bool((w[:N] < 1 << 20).all()), '%s: an element was not written' % k
            assert N % 2 == 0 or int(w[N]) == POISON_HI, '%s: written past its end' % k     # ... and the half behind an odd N is


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _steps_of(job, i):
    na = int(job['n_acc'][i])
    r = job['rec'][:na, :, i].cpu()
    return [(float(a), float(b)) for a, b in r]


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('net', range(len(NETS)))
def test_every_path_against_the_restatement_alone(net, N):
    from xnode_wan_pde_solver_amd import kernels as KN, evalpaths as EP
    d, H, K, m = NETS[net]
    theta, blob_h = _theta(H, K, m, d, 500 + net)
    x, start, t_in, t_end, big = (a[:N] for a in _paths(d, SEEDS[net]))
    ref = _free(net)[:N]
    dev = torch.device('cuda')
    arena = G.Arena(dev)
    with arena.workspaces(KN):
        blob = arena.inp(blob_h, name='theta')
        full = _launch(KN, arena, blob, x, start, t_in, t_end, H, K, m)
        bare = _launch(KN, arena, blob, x, start, t_in, t_end, H, K, m, want_Y=False, cap=0, want_fin=False)
        short = _launch(KN, arena, blob, x, start, t_in, t_end, H, K, m, cap=2)
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(100 * net + N))
        moved = _launch(KN, arena, blob, x[perm], start[perm], t_in[perm], t_end[perm], H, K, m)
        chunked = EP.paths_dopri5(full['xT'], full['t_in'], full['t_end'], full['start'], blob, H, K, m, H, KN.DOPRI5_RTOL,
                                  KN.DOPRI5_ATOL, chunk=16)
    # (4) every output element written, no guard element touched -- the workspaces' included
    _check_written(arena, (full, bare, short, moved))
    what = 'net %s N %d' % (NETS[net], N)
    assert not bool(full['status'].any()), what
    n_acc, n_att = full['n_acc'].cpu(), full['n_att'].cpu()
    assert int(n_acc.max()) < CAP                                    # (the record holds every step of every path)
    if N > 2:                                                        # no step beside many, and the large start's own count, in one tile
        assert int(n_att[1]) == 0 and len({int(n_att[0]), int(n_att[1]), int(n_att[2])}) == 3, what
    # (3) the same bits: without Y / rec / fin, with a short record, beside other neighbours, in chunks of 16
    pd = perm.to(dev)
    for k in ('u', 'status', 'n_acc', 'n_att'):
        assert torch.equal(bare[k], full[k]) and torch.equal(short[k], full[k]), k + ' ' + what
        assert torch.equal(moved[k], full[k][pd]), 'permuted ' + k + ' ' + what
        assert torch.equal(chunked[k].to(dev), full[k]), 'chunked ' + k + ' ' + what
    assert torch.equal(short['Y'], full['Y']) and torch.equal(short['fin'], full['fin']) and torch.equal(chunked['fin'], full['fin'])
    assert torch.equal(moved['Y'], full['Y'][:, pd]) and torch.equal(moved['fin'], full['fin'][:, pd])
    keep = (torch.arange(2, device=dev).view(2, 1, 1) < full['n_acc'].view(1, 1, N)).expand(2, 2, N)
    assert torch.equal(short['rec'][keep], full['rec'][:2][keep]), 'short record ' + what
    keep = (torch.arange(CAP, device=dev).view(CAP, 1, 1) < full['n_acc'].view(1, 1, N)).expand(CAP, 2, N)
    assert torch.equal(moved['rec'][keep[:, :, pd]], full['rec'][:, :, pd][keep[:, :, pd]]), 'permuted record ' + what
    # fin: where the controller stopped -- the end of the last accepted step
    u, Y = full['u'].cpu(), full['Y'].cpu()
    worst = dict(grid=0.0, Y=0.0, u=0.0, Yfree=0.0)
    for i in range(N):
        y_r, u_r, info = ref[i]
        steps = _steps_of(full, i)
        if steps:
            assert float(full['fin'][0, i]) == steps[-1][0] + steps[-1][1] >= float(t_end[i]) > steps[-1][0], (what, i)
        else:
            assert float(full['fin'][0, i]) == float(t_in[i]) == float(t_end[i]), (what, i)
        if m == 1:
            # (1) tanh-only field: the step decisions, the grid, u and Y against the free-running restatement
            assert info['gap'] > 1e-9, 'bad fixture: path %d has a step decision within %.1e of the threshold' % (i, info['gap'])
            cond = max([c for c, free in info['cond'] if free] or [0.0])
            assert cond <= COND_MAX, 'bad fixture: path %d has an error ratio of condition number %.1e' % (i, cond)
            assert (int(n_att[i]), int(n_acc[i])) == (info['n_att'], info['n_acc']), (what, i)
            if steps:
                worst['grid'] = max(worst['grid'], _rel(torch.tensor(steps, dtype=F64), torch.tensor(info['steps'], dtype=F64)))
            y_c = y_r
        else:
            # (2) ReLU layers: against the restatement on the path's own recorded steps; the free-running one within tolerance
            y_c, u_r, _ = _frozen(net, i, steps)
            assert int(n_att[i]) >= int(n_acc[i]) and abs(int(n_acc[i]) - info['n_acc']) <= max(3, info['n_acc'] // 5), (what, i)
            worst['Yfree'] = max(worst['Yfree'], _rel(Y[:, i], y_r))
        worst['Y'] = max(worst['Y'], _rel(Y[:, i], y_c))
    u_c = torch.tensor([ref[i][1] if m == 1 else _frozen(net, i, _steps_of(full, i))[1] for i in range(N)], dtype=F64)
    for grp in (big, ~big):
        if bool(grp.any()):
            worst['u'] = max(worst['u'], _rel(u[grp], u_c[grp]))
    print('%s: attempts %d..%d, accepted %d..%d; worst grid %.2e Y %.2e u %.2e Y against the free restatement %.2e'
          % (what, int(n_att.min()), int(n_att.max()), int(n_acc.min()), int(n_acc.max()), worst['grid'], worst['Y'], worst['u'],
             worst['Yfree']))
    assert worst['grid'] < GRID_TOL and worst['Y'] < TOL and worst['u'] < TOL and worst['Yfree'] < TOL_FREE, what


def test_graph_replay_gives_the_same_bits():
    from xnode_wan_pde_solver_amd import kernels as KN
    net, N = 3, NMAX
    d, H, K, m = NETS[net]
    _, blob_h = _theta(H, K, m, d, 500 + net)
    x, start, t_in, t_end, _ = _paths(d, SEEDS[net])
    dev = torch.device('cuda')
    outs = dict(u=torch.empty(N, dtype=F64, device=dev), Y=torch.empty(H, N, dtype=F64, device=dev),
                rec=torch.empty(CAP, 2, N, dtype=F64, device=dev), fin=torch.empty(2, N, dtype=F64, device=dev),
                status=torch.empty(N, dtype=I32, device=dev), n_acc=torch.empty(N, dtype=I32, device=dev),
                n_att=torch.empty(N, dtype=I32, device=dev))
    job = dict(outs, xT=x.t().contiguous().to(dev), start=start.to(dev), t_in=t_in.to(dev), t_end=t_end.to(dev))
    blob = blob_h.to(dev)
    outs['rec'].zero_()
    KN.paths_dopri5_fwd([job], blob, H, K, m, H)
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in outs.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        KN.paths_dopri5_fwd([job], blob, H, K, m, H)           # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k, v in outs.items():
        v.zero_() if k == 'rec' else v.fill_(-1)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        KN.paths_dopri5_fwd([job], blob, H, K, m, H)
    g.replay()
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert torch.equal(v, first[k]), k


@pytest.mark.parametrize('net', (0, 3))
def test_limits_stop_exactly_the_paths_that_need_more(net):
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m = NETS[net]
    _, blob_h = _theta(H, K, m, d, 500 + net)
    x, start, t_in, t_end, _ = _paths(d, SEEDS[net])
    dev = torch.device('cuda')
    arena = G.Arena(dev)
    with arena.workspaces(KN):
        blob = arena.inp(blob_h, name='theta')
        free = _launch(KN, arena, blob, x, start, t_in, t_end, H, K, m)
        # (max_attempts given: its default, 2 max_steps = 4 rounds, would end paths that reject twice before their second step)
        two = _launch(KN, arena, blob, x, start, t_in, t_end, H, K, m, max_steps=2, max_attempts=1000)
        three = _launch(KN, arena, blob, x, start, t_in, t_end, H, K, m, max_attempts=3)
    _check_written(arena, (free, two, three))
    assert not bool(free['status'].any())
    more = free['n_acc'] > 2
    assert 0 < int(more.sum()) < NMAX and bool(more[:16].any()) and not bool(more[:16].all())      # both kinds in one tile
    assert torch.equal(two['status'], torch.where(more, STEPS, 0).to(I32))
    assert bool((two['n_acc'][more] == 2).all())
    for k in ('u', 'n_acc', 'n_att'):
        assert torch.equal(two[k][~more], free[k][~more]), k
    assert torch.equal(two['Y'][:, ~more], free['Y'][:, ~more])
    # (the first two steps of every path: the same decisions; compared as bit patterns, unwritten slots hold the poison in both)
    assert torch.equal(two['rec'][:2].view(torch.int64), free['rec'][:2].view(torch.int64))
    more = free['n_att'] > 3
    assert 0 < int(more.sum()) < NMAX
    assert torch.equal(three['status'], torch.where(more, STEPS, 0).to(I32))
    assert bool((three['n_att'][more] == 3).all())
    for k in ('u', 'n_acc', 'n_att'):
        assert torch.equal(three[k][~more], free[k][~more]), k
    assert torch.equal(three['Y'][:, ~more], free['Y'][:, ~more])


def test_wrapper_refusals():
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    d, H, K, m = NETS[0]
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 1)
    z = torch.zeros(5, dtype=F64, device=dev)
    i = torch.zeros(5, dtype=I32, device=dev)
    job = dict(xT=torch.zeros(d, 5, dtype=F64, device=dev), start=z, t_in=z, t_end=z, u=z.clone(), status=i, n_acc=i.clone(), n_att=i.clone())
    with pytest.raises(XnwanError, match='status must be'):
        KN.paths_dopri5_fwd([dict(job, status=z)], blob.to(dev), H, K, m, H)
    with pytest.raises(XnwanError, match='needs n_att'):
        KN.paths_dopri5_fwd([{k: v for k, v in job.items() if k != 'n_att'}], blob.to(dev), H, K, m, H)
    with pytest.raises(XnwanError, match='rec must have shape'):
        KN.paths_dopri5_fwd([dict(job, rec=torch.zeros(4, 5, dtype=F64, device=dev))], blob.to(dev), H, K, m, H)
    with pytest.raises(XnwanError, match='max_attempts'):
        KN.paths_dopri5_fwd([job], blob.to(dev), H, K, m, H, max_attempts=0)
    with pytest.raises(XnwanError, match='XW_E_ARG'):
        KN.paths_dopri5_fwd([job], blob.to(dev), H, K, m, H + 1)


# ---- the public surface ----------------------------------------------------------------------------------------------------------------
SURFACE = [('Hypercube', 'Ex4_1', 20, 10, 1), ('NSphere_THourglass', 'Ex4_3', 65, 16, 1), ('Hypercube', 'Ex4_1', 20, 10, 8),
           ('NSphere_THourglass', 'Ex4_3', 20, 10, 8)]
M_POINTS = 50


def _dopri5_solver(domain, P, H, K, m):
    from test_gpu_eval_paths import _solver
    from xnode_wan_pde_solver_amd.options import EngineOptions
    from xnode_wan_pde_solver_amd import kernels as KN
    tiled = KN.stepper_family(H, K, m) == 'tiled'
    return _solver(domain, P, H, K, m, 'dopri5', options=EngineOptions(dopri5_stepper='tiled') if tiled else None)


def _surface(domain, P, H, K, m):
    """(evaluate, module, params, theta).  The cube: NODE_WAN_solver.evaluate.  The hourglass: NODE_WAN_solver refuses to TRAIN
    dopri5 on the ball domains (their groups start inside the interval), so what it evaluates with, the bound XNODE module with the
    domain's `entry` rule, is built directly -- XNODE.evaluate is what NODE_WAN_solver.evaluate calls"""
    from test_gpu_eval_paths import _theta_of
    from oracle import refspec as R
    from xnode_wan_pde_solver_amd import kernels as KN, nets, sampling
    if domain == 'Hypercube':
        S, params = _dopri5_solver(domain, P, H, K, m)
        return S.evaluate, S.u_net.module, params, _theta_of(S, m)
    params = {'u_layers': m, 'u_hidden_dim': H, 'u_hidden_hidden_dim': K, 'solver': 'dopri5', 'dim': 3, 'N_t': 6, 'T0': 0, 'T': 1,
              'shape_param': 1.0}
    torch.manual_seed(11)
    net = nets.XNODE(H, 1, P.func_h, P.func_g, params, K, m, sampling.resolve_domain(domain), solver='dopri5')
    with torch.no_grad():                                        # non-zero biases: every bias path is exercised
        for p in net.parameters():
            if p.dim() == 1:
                p.copy_(0.3 * torch.randn(p.shape, dtype=F64))
    if KN.stepper_family(H, K, m) == 'tiled':
        net.dopri5_stepper = 'tiled'
    net.bind(torch.device('cuda'))
    named = dict(net.named_parameters())
    theta = {k: named[nm[len('module.'):]].detach().cpu().clone() for nm, k in R.u_names(m)}
    if m == 1:
        theta['Wh'], theta['Wh_b'] = torch.zeros(K, K, dtype=F64), torch.zeros(K, dtype=F64)
    return net.evaluate, net, params, theta


def _reference(points, domain, params, theta, P):
    """per point, on the CPU: entry by the domain's rule (restated), dopri5_ref.u_net on the one-path group [[t_in, x], [t, x]] with
    the start value of the same callables: (u [M], min gap)"""
    T0, T = params['T0'], params['T']
    out, gap = [], float('inf')
    for p in points:
        t, x = float(p[0]), p[1:]
        t_in, boundary = float(T0), False
        if domain == 'NSphere_THourglass':
            rad, half = float(torch.sqrt(torch.sum(x ** 2))), (T - T0) / 2
            if not (t < half or rad <= params['shape_param'] * half):
                t_in, boundary = rad / params['shape_param'], True
        X = torch.cat((torch.tensor([t_in, t], dtype=F64).view(1, 2, 1), x.view(1, 1, -1).expand(1, 2, -1)), 2)
        s = P.func_g(X[:, :1, :]).reshape(-1) if boundary else P.func_h(X[:, 0, :]).reshape(-1)
        u, info = D.u_net(theta, params, X, s)
        out.append(u.reshape(-1)[-1])
        gap = min(gap, info['gap'])
    return torch.stack(out), gap


@pytest.mark.parametrize('domain,funcs,H,K,m', SURFACE)
def test_solver_evaluate_with_dopri5_matches_a_per_point_reference(domain, funcs, H, K, m):
    from test_gpu_eval_paths import _eval_points
    P = importlib.import_module('configs.%s_funcs' % funcs)
    evaluate, module, params, theta = _surface(domain, P, H, K, m)
    pts = _eval_points(domain, M=M_POINTS)
    u = evaluate(pts)                                            # host points, float64
    assert u.shape == (M_POINTS,) and u.dtype == F64 and u.is_cuda and not u.requires_grad
    want, gap = _reference(pts, domain, params, theta, P)
    err = _rel(u, want)
    print('evaluate %s (%d, %d, %d): rel-to-scale error %.2e, min gap %.2e' % (domain, H, K, m, err, gap))
    if m == 1:
        assert gap > 1e-9, 'bad fixture: a step decision within %.1e of the threshold' % gap
    tol = TOL if m == 1 else TOL_FREE
    assert err < tol
    # device points, the module's own entry point: h and g are then evaluated on the device (their last bits may differ)
    assert _rel(module.evaluate(pts.cuda()), want) < tol
    assert torch.equal(module.evaluate(pts, chunk=16), u)
    p32 = pts.float()                                            # float32 points are widened exactly
    assert torch.equal(evaluate(p32), evaluate(p32.double()))
    if domain == 'NSphere_THourglass':
        from xnode_wan_pde_solver_amd import sampling
        t_in, at_T0 = sampling.NSphere_THourglass.entry(pts, params['shape_param'], 0, 1)
        assert 0 < int(at_T0.sum()) < M_POINTS and float(t_in[5]) == float(pts[5, 0])        # late entries, and t == t_in


def test_evaluate_names_the_first_point_at_the_step_limit():
    import configs.Ex4_1_funcs as P
    from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    S, params = _dopri5_solver('Hypercube', P, 20, 10, 8)
    from test_gpu_eval_paths import _eval_points
    pts = _eval_points('Hypercube', M=M_POINTS)
    pts[0, 0] = 0.0                                              # t == t_in: no step, never at the limit
    net = S.u_net.module
    dev = net.blob.data.device
    first = torch.cat((torch.zeros(M_POINTS, 1, dtype=F64), pts[:, 1:]), 1)
    r = EP.paths_dopri5(pts[:, 1:].t().contiguous().to(dev), torch.zeros(M_POINTS, dtype=F64, device=dev), pts[:, 0].contiguous().to(dev),
                        P.func_h(first).reshape(-1).double().to(dev), net.blob.data, net.kdims[0], net.kdims[1], 8, 20,
                        KN.DOPRI5_RTOL, KN.DOPRI5_ATOL, max_steps=1)
    # the points as the caller numbers them, unsorted, under the same limits (one accepted step, two rounds): who stops is the
    # kernel's to say (test_limits_... pins it); evaluate() must name the first of them and count them through its sort
    more = (r['status'] != 0).nonzero().view(-1)
    assert bool((r['status'][more] == STEPS).all()) and 0 < more.numel() < M_POINTS and int(more[0]) > 0
    with pytest.raises(XnwanError, match='step limit of 1 accepted steps') as e:
        net.evaluate(pts, max_steps=1)
    assert '%d of %d points' % (more.numel(), M_POINTS) in str(e.value) and 'first: point %d,' % int(more[0]) in str(e.value)
    with pytest.raises(XnwanError, match="n_sub = 3 with solver 'dopri5'"):
        S.evaluate(pts, n_sub=3)


def test_midpoint_evaluate_returns_the_bits_of_the_per_path_kernel():
    """evaluate with a fixed-grid solver is what it was: the grids of evalpaths on kernels.tiled_paths_fwd, directly"""
    import configs.Ex4_3_funcs as P
    from test_gpu_eval_paths import _eval_points, _solver
    from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN, sampling
    S, params = _solver('NSphere_THourglass', P, 20, 10, 8, 'midpoint')
    pts = _eval_points('NSphere_THourglass', M=M_POINTS)
    u = S.evaluate(pts)
    net = S.u_net.module
    dev = net.blob.data.device
    t = pts[:, 0].contiguous()
    t_in, at_T0 = sampling.NSphere_THourglass.entry(pts, params['shape_param'], 0, 1)
    first = torch.cat((t_in.view(-1, 1), pts[:, 1:]), 1)
    s = torch.where(at_T0, P.func_h(first).reshape(-1).double(), P.func_g(first.unsqueeze(1)).reshape(-1).double())
    n = EP.step_counts(t, t_in, 0, 1, params['N_t'])
    order, inverse = EP.sort_by_steps(n)
    job = dict(xT=pts[order, 1:].t().contiguous().to(dev), start=s[order].contiguous().to(dev),
               tT=EP.pack_grids(t[order], t_in[order], n[order]).to(dev), nstep=n[order].to(I32).to(dev),
               u=torch.empty(M_POINTS, dtype=F64, device=dev))
    KN.tiled_paths_fwd([job], net.blob.data, KN.METHODS['midpoint'], net.kdims[0], net.kdims[1], 8, last_only=True)
    assert torch.equal(u, job['u'][inverse.to(dev)])
