"""The tangent of the slab-writing sweep over a ragged group (csrc/xw_tiled_paths_gvjp.hip: kt_paths_gvjp) and the parameter
gradients of u, du/dx and ut at scattered points built on it (kernels.tiled_paths_gvjp, evalpaths.evaluate_points_grad_vjp,
XNODE.evaluate_grad_vjp / evaluate_grad_fn, NODE_WAN_solver.evaluate_grad_vjp) on the device.

Kernel level, inside the guard-banded, poisoned arena of tests/guarded.py with the workspace handed in guarded, at the shapes of
tests/test_gpu_eval_paths.py (its _ragged: a path without a step beside one with L - 1 in one tile; every path a start time of its
own): slab_sum(gslab) against oracle.refspec run on every path ALONE under autograd -- reverse over reverse in (x, s) then theta,
ut from refspec.field at the path's end (tests/grad_vjp_oracle.py) -- summed with the weights on the host, below 1e-10 of the scale
of each parameter block (TOL_G of tests/test_gpu_eval_vjp.py and tests/test_gpu_eval_hess.py, which bound the same block
arithmetic; the oracle's own two routes agree to 1e-15, tests/test_eval_grad_vjp_host.py), Win cut into its x, time and y columns.
Zeros are never compared with a relative bound: a block the oracle gives as identically zero for a structural reason must be exact
zeros on the device, and the oracle is asserted to be identically zero there.  The structural cases (_structural_zeros):
  * Wh, Wh_b at m = 1: the network has no hidden layer, the slot is unused
  * every block of the field (Win's three parts, Win_b, Wh, Wh_b, Wo, Wo_b) where no path takes a step (L == 1) and wt is absent:
    only ut evaluates the field there
  * FL_b when wu is absent: the direction's term and ut do not see the read-out's bias
  * the lift's biases IL0_b, IL2_b, IL4_b where no path takes a step and wu and wt are absent: the direction's term is then
    FL_w . d lift(s)/ds vs, and the lift is piecewise linear -- its derivative in s does not depend on its biases
  * Wo_b under the direction alone where no path takes more than ONE euler step (L == 2): y_1 = y_0 + dt F(t_0, x, y_0) carries
    Wo_b as a constant, which a derivative in (x, s) does not see; a second step, or midpoint's and rk4's second stage, evaluates
    the field at a state that holds it
Each term alone (wu against tiled_paths_vjp below 1e-12, wt and the direction against the oracle), their sum against the combined
launch; the bits with and without the nstep hint, launched twice, replayed from a captured graph, doubled, under one-hot weights,
with zero weights on the stepless path; a permutation below 1e-12; every element of gslab written, no guard touched, every input
bit-unchanged.  Public surface: solver.evaluate_grad_vjp on the cube, the cone and the hourglass's T0-entered points against a
per-point CPU loop over oracle.refspec.u_net with h([T0, x]) in the graph of x; chunks; evaluate_grad_fn under torch.autograd.grad
and torch.optim.SGD; the refusals."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402
import grad_vjp_oracle as O  # noqa: E402
from test_gpu_tiled_stepper import F64, U_ORDER, _close, _theta  # noqa: E402
from test_gpu_eval_paths import METHODS, NETS, _eval_points, _ragged, _solver, _theta_of  # noqa: E402
from test_gpu_eval_grad import _forward  # noqa: E402
from test_gpu_eval_vjp import _blocks, _entered_at_T0  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_G, TOL_T = 1e-10, 1e-12
NS, LS = (1, 17, 37), (1, 2, 5)
FIELD = ('Win[:, :d]', 'Win[:, d]', 'Win[:, d+1:]', 'Win_b', 'Wh', 'Wh_b', 'Wo', 'Wo_b')
_ORACLE = {}
assert U_ORDER == O.U_ORDER


def _rand(shape, seed):
    w = torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))
    assert bool((w != 0).all())
    return w


def _oracle_alone(theta, m, method, x, start, n, tT, vx, vs, key):
    """per path ALONE over its own n_i + 1 times: (Gu, Gd, Gt), each [N, P_u] -- the gradients in theta of U, of its derivative along
    (vx_i, vs_i) and of ut, unweighted.  Computed once per case and left unchanged"""
    if key not in _ORACLE:
        rows = [tuple(O.flat(g) for g in O.reverse_over_reverse(theta, m, method, x[i], start[i], tT[:int(n[i]) + 1, i], vx[i], vs[i]))
                for i in range(x.shape[0])]
        _ORACLE[key] = tuple(torch.stack([r[k] for r in rows]) for k in range(3))
    return _ORACLE[key]


def _ref(Gs, wu=None, c=None, wt=None):
    """sum_p wu_p Gu_p + c_p Gd_p + wt_p Gt_p (c: the factor on path p's direction; None: the term is absent)"""
    out = torch.zeros(Gs[0].shape[1], dtype=F64)
    for w, Gm in zip((wu, c, wt), Gs):
        if w is not None:
            out = out + (w.view(-1, 1) * Gm).sum(0)
    return out


def _structural_zeros(m, method, nmax, has_u, has_d, has_t):
    """the blocks that vanish identically on a group whose longest path takes nmax steps, under the terms present"""
    z = set()
    if m == 1:
        z |= {'Wh', 'Wh_b'}
    if nmax == 0 and not has_t:
        z |= set(FIELD)
    if not has_u:
        z.add('FL_b')
    if not has_u and not has_t:
        if nmax == 0:
            z |= {'IL0_b', 'IL2_b', 'IL4_b'}
        if nmax == 1 and method == 'euler':
            z.add('Wo_b')
    return z


def _check_blocks(got, ref, blocks, zeros, what, record=None):
    """got against ref block by block, 1e-10 of each block's own scale; the blocks of `zeros` are identically zero in the oracle and
    exact zeros on the device; no other block of the oracle may vanish"""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    for name, idx in blocks.items():
        g, r = got[idx], ref[idx]
        if name in zeros:
            assert bool((r == 0).all()), 'the oracle is not identically zero: %s %s' % (name, what)
            assert bool((g == 0).all()), 'exact zeros expected: %s %s' % (name, what)
            continue
        scale = float(r.abs().max())
        assert scale > 0, 'a comparison of zeros: %s %s' % (name, what)
        err = float((g - r).abs().max()) / scale
        if record is not None:
            record[name] = max(record.get(name, 0.0), err)
        assert err < TOL_G, '%s %s: max rel-to-scale error %.3e (scale %.3e)' % (name, what, err, scale)


def _tangent(KN, arena, blob, fj, vx, vs, H, K, m, mid):
    """the guarded tangent forward (tiled_paths_hvp with ju alone) for the direction (vx [N, d], vs [N], host): the job's direction
    part -- vx [d, N], vs, Yd -- as views of the arena"""
    d, N = fj['xT'].shape
    L = fj['tT'].shape[0]
    o = dict(vx=arena.inp(vx.t(), name='vx'), vs=arena.inp(vs, name='vs'), Yd=arena.out(L, H, N, name='Yd'))
    job = dict({k: fj[k] for k in ('xT', 'start', 'tT', 'Y', 'nstep')}, ju=arena.out(N, name='ju'), **o)
    work = arena.out(KN.lib.xw_paths_tiled_hvp_work(d, H, K, m) * ((N + 15) // 16), name='hvp_work')
    KN.tiled_paths_hvp([job], blob, mid, H, K, m, work=work)
    return o


def _gvjp(KN, arena, blob, fj, H, K, m, mid, wu=None, dirn=None, wt=None, hint=True):
    """one guarded launch of the sweep on the forward job fj with the weights wu, wt (host, or None) and the direction part dirn
    (_tangent's, or None): the job with its slabs and the slabs' sum (outside the arena)"""
    d, N = fj['xT'].shape
    tiles = (N + 15) // 16
    job = {k: fj[k] for k in ('xT', 'start', 'tT', 'Y')}
    if hint and 'nstep' in fj:
        job['nstep'] = fj['nstep']
    if wu is not None:
        job['wu'] = arena.inp(wu, name='wu')
    if wt is not None:
        job['wt'] = arena.inp(wt, name='wt')
    if dirn is not None:
        job.update(dirn)
    job['gslab'] = arena.out(tiles, blob.numel(), name='gslab')
    work = arena.out(KN.lib.xw_paths_tiled_gvjp_work(d, H, K, m) * tiles, name='gvjp_work')
    KN.tiled_paths_gvjp([job], blob, mid, H, K, m, work=work)
    job['gflat'] = KN.slab_sum(job['gslab'])
    return job


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('net', range(len(NETS)))
@pytest.mark.parametrize('method', METHODS)
def test_per_path_tangent_sweep_with_slabs(method, net, N):
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
        wu, wt, vx, vs = _rand((N,), seed + 5), _rand((N,), seed + 6), _rand((N, d), seed + 7), _rand((N,), seed + 8)
        assert int(n.max()) == L - 1
        if L == 5 and N > 1:
            assert int(n[0]) == 0 and int(n[1]) == 4                 # no step beside four, in one tile
            assert float((tT[0] - tT[0, 0]).abs().max()) > 0.01      # a start time per path: a tile-wide t fails the time column
        arena = G.Arena(dev)
        with arena.workspaces(KN):
            blob = arena.inp(blob_h, name='theta')
            fj = _forward(KN, arena, blob, x, start, tT, n, H, K, m, mid)
            dn = _tangent(KN, arena, blob, fj, vx, vs, H, K, m, mid)
            torch.cuda.synchronize()
            kept = {k: fj[k].clone() for k in ('xT', 'start', 'tT', 'Y', 'nstep')}
            kept.update({k: dn[k].clone() for k in dn}, theta=blob.clone())
            plain = _gvjp(KN, arena, blob, fj, H, K, m, mid, wu, dn, wt, hint=False)
            kept.update(wu=plain['wu'].clone(), wt=plain['wt'].clone())
            hinted = _gvjp(KN, arena, blob, fj, H, K, m, mid, wu, dn, wt)
            again = _gvjp(KN, arena, blob, fj, H, K, m, mid, wu, dn, wt, hint=False)
            dn2 = _tangent(KN, arena, blob, fj, 2 * vx, 2 * vs, H, K, m, mid)
            twice = _gvjp(KN, arena, blob, fj, H, K, m, mid, 2 * wu, dn2, 2 * wt)
            only_u = _gvjp(KN, arena, blob, fj, H, K, m, mid, wu=wu)
            only_d = _gvjp(KN, arena, blob, fj, H, K, m, mid, dirn=dn)
            only_t = _gvjp(KN, arena, blob, fj, H, K, m, mid, wt=wt)
            # kt_paths_vjp's text of the wu term
            vj = dict({k: fj[k] for k in ('xT', 'start', 'tT', 'Y', 'nstep')}, w=only_u['wu'],
                      gslab=arena.out((N + 15) // 16, blob.numel(), name='vjp_gslab'))
            KN.tiled_paths_vjp([vj], blob, mid, H, K, m,
                               work=arena.out(KN.lib.xw_paths_tiled_vjp_work(d, H, K, m) * ((N + 15) // 16), name='vjp_work'))
            vj['gflat'] = KN.slab_sum(vj['gslab'])
            # zero weights and a zero direction on path 0 (it takes no step where N > 1)
            keep = torch.ones(N, dtype=F64)
            keep[0] = 0.0
            dn0 = _tangent(KN, arena, blob, fj, keep.view(-1, 1) * vx, keep * vs, H, K, m, mid)
            muted = _gvjp(KN, arena, blob, fj, H, K, m, mid, keep * wu, dn0, keep * wt)
            perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed + 1))
            fm = _forward(KN, arena, blob, x[perm], start[perm], tT[:, perm].contiguous(), n[perm], H, K, m, mid)
            dm = _tangent(KN, arena, blob, fm, vx[perm], vs[perm], H, K, m, mid)
            moved = _gvjp(KN, arena, blob, fm, H, K, m, mid, wu[perm], dm, wt[perm])
        # every element of gslab written, no guard element touched (the workspaces' included); the inputs hold their bits
        jobs = [plain, hinted, again, twice, only_u, only_d, only_t, muted, moved, vj]
        arena.check(written=[j['gslab'] for j in jobs] + [fj['Y'], fm['Y'], dn['Yd'], dn2['Yd'], dn0['Yd'], dm['Yd']])
        what = '%s %s N %d L %d' % (method, NETS[net], N, L)
        for k in ('xT', 'start', 'tT', 'Y', 'nstep'):
            assert torch.equal(fj[k], kept[k]), '%s changed: %s' % (k, what)
        for k in ('vx', 'vs', 'Yd'):
            assert torch.equal(dn[k], kept[k]), '%s changed: %s' % (k, what)
        assert torch.equal(blob, kept['theta']) and torch.equal(plain['wu'], kept['wu']) and torch.equal(plain['wt'], kept['wt']), what
        # 1. the oracle: every path alone, summed with the weights on the host
        Gs = _oracle_alone(theta, m, method, x, start, n, tT, vx, vs, (method, net, N, L))
        one = torch.ones(N, dtype=F64)
        _check_blocks(plain['gflat'], _ref(Gs, wu, one, wt), blocks, _structural_zeros(m, method, L - 1, True, True, True), what, worst)
        # 2. each term alone, and their sum
        _check_blocks(only_u['gflat'], _ref(Gs, wu=wu), blocks, _structural_zeros(m, method, L - 1, True, False, False), 'wu alone ' + what)
        _check_blocks(only_d['gflat'], _ref(Gs, c=one), blocks, _structural_zeros(m, method, L - 1, False, True, False), 'direction alone ' + what)
        _check_blocks(only_t['gflat'], _ref(Gs, wt=wt), blocks, _structural_zeros(m, method, L - 1, False, False, True), 'wt alone ' + what)
        _close(only_u['gflat'], vj['gflat'], TOL_T, 'wu alone against tiled_paths_vjp ' + what)
        _close(only_u['gflat'] + only_d['gflat'] + only_t['gflat'], plain['gflat'], TOL_T, 'the three terms summed ' + what)
        # 3. bits: the hint, the same launch twice, everything doubled
        for other, name in ((hinted, 'nstep'), (again, 'again')):
            assert torch.equal(other['gslab'], plain['gslab']), '%s gslab %s' % (name, what)
        assert torch.equal(dn2['Yd'], 2 * dn['Yd']), 'Yd of twice the direction ' + what
        assert torch.equal(twice['gslab'], 2 * plain['gslab']), 'doubled %s' % what
        # zero weights on path 0: the other tiles' bits as they were, the sum still the oracle's
        assert torch.equal(muted['gslab'][1:], hinted['gslab'][1:]), what
        if N > 1:
            _check_blocks(muted['gflat'], _ref(Gs, keep * wu, keep, keep * wt), blocks, _structural_zeros(m, method, L - 1, True, True, True),
                          'path 0 muted ' + what)
        else:
            assert bool((muted['gslab'] == 0).all()), 'a path without weights and direction adds exact zeros: ' + what
        # a permutation of the paths with their weights: the sum in another order
        _close(moved['gflat'], plain['gflat'], TOL_T, 'permuted gflat ' + what)
    print('largest error against the oracle per block, %s %s N %d: %s'
          % (method, NETS[net], N, ', '.join('%s %.1e' % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize('N', (17, 37))
@pytest.mark.parametrize('method', METHODS)
def test_one_hot_weights_give_that_paths_own_launch(method, N):
    """neighbours and padding lanes add exact zeros: the slab sum under weights and a direction on path i alone is, to the bit, the
    slab sum of the N = 1 launch of that path"""
    from xnode_wan_pde_solver_amd import kernels as KN
    dev = torch.device('cuda')
    L = 5
    for net, (d, H, K, m) in enumerate(NETS):
        mid = KN.method_id(method)
        _, blob_h = _theta(H, K, m, d, 300 + net)
        x, start, n, tT = _ragged(N, L, d, 77 + N + net)
        wu, wt, vx, vs = _rand((N,), 78 + N), _rand((N,), 79 + N), _rand((N, d), 80 + N), _rand((N,), 81 + N)
        arena = G.Arena(dev)
        written = []
        with arena.workspaces(KN):
            blob = arena.inp(blob_h, name='theta')
            fj = _forward(KN, arena, blob, x, start, tT, n, H, K, m, mid)
            for i in (0, 1, 16, N - 1):
                hot = torch.zeros(N, dtype=F64)
                hot[i] = 1.0
                dh = _tangent(KN, arena, blob, fj, hot.view(-1, 1) * vx, hot * vs, H, K, m, mid)
                full = _gvjp(KN, arena, blob, fj, H, K, m, mid, hot * wu, dh, hot * wt)
                f1 = _forward(KN, arena, blob, x[i:i + 1], start[i:i + 1], tT[:, i:i + 1].contiguous(), n[i:i + 1], H, K, m, mid)
                d1 = _tangent(KN, arena, blob, f1, vx[i:i + 1], vs[i:i + 1], H, K, m, mid)
                alone = _gvjp(KN, arena, blob, f1, H, K, m, mid, wu[i:i + 1], d1, wt[i:i + 1])
                written += [full['gslab'], alone['gslab'], f1['Y'], dh['Yd'], d1['Yd']]
                what = '%s %s N %d path %d' % (method, NETS[net], N, i)
                assert float(alone['gflat'].abs().max()) > 0, what
                assert torch.equal(full['gflat'], alone['gflat']), what
                for k in range((N + 15) // 16):                    # the tiles that hold no weight keep the entry point's zeros
                    if k != i // 16:
                        assert bool((full['gslab'][k] == 0).all()), what
        arena.check(written=written + [fj['Y']])


def test_graph_replay():
    """a captured launch (the slabs' zeroing and the sweep) replays to the same bits"""
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m = NETS[2]
    N, L = 37, 5
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 7)
    x, start, n, tT = _ragged(N, L, d, 8)
    bc = blob.to(dev)
    new = lambda *shape: torch.empty(*shape, dtype=F64, device=dev)   # noqa: E731
    job = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), tT=tT.to(dev), nstep=n.to(torch.int32).to(dev), u=new(L, N),
               Y=new(L, H, N), vx=_rand((d, N), 9).to(dev), vs=_rand((N,), 10).to(dev), Yd=new(L, H, N))
    KN.tiled_paths_fwd([job], bc, 2, H, K, m)
    KN.tiled_paths_hvp([dict(job, ju=new(N))], bc, 2, H, K, m)
    job = dict({k: v for k, v in job.items() if k != 'u'}, wu=_rand((N,), 11).to(dev), wt=_rand((N,), 12).to(dev), gslab=new(3, bc.numel()))
    work = KN.paths_gvjp_work(d, H, K, m, 3, dev)
    KN.tiled_paths_gvjp([job], bc, 2, H, K, m, work=work)
    first = job['gslab'].clone()
    assert float(first.abs().max()) > 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        KN.tiled_paths_gvjp([job], bc, 2, H, K, m, work=work)     # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    job['gslab'].fill_(float('nan'))
    with torch.cuda.graph(g):
        KN.tiled_paths_gvjp([job], bc, 2, H, K, m, work=work)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(job['gslab'], first)


def test_kernel_wrapper_refusals():
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    d, H, K, m = NETS[0]
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 1)
    bc = blob.to(dev)
    x, start, n, tT = _ragged(5, 3, d, 2)
    z = lambda *shape: torch.zeros(*shape, dtype=F64, device=dev)   # noqa: E731
    job = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), tT=tT.to(dev), Y=z(3, H, 5), Yd=z(3, H, 5), vx=z(d, 5), vs=z(5),
               wu=z(5), wt=z(5), gslab=z(1, bc.numel()))
    for mid in (KN.DOPRI5, KN.ADAMS):
        with pytest.raises(XnwanError, match='fixed-grid'):
            KN.tiled_paths_gvjp([job], bc, mid, H, K, m)
    for k in ('Y', 'gslab', 'Yd'):
        with pytest.raises(XnwanError, match='tiled_paths_gvjp: ' + k):
            KN.tiled_paths_gvjp([{a: v for a, v in job.items() if a != k}], bc, 0, H, K, m)
    for k in ('vx', 'vs'):
        with pytest.raises(XnwanError, match='both or neither'):
            KN.tiled_paths_gvjp([{a: v for a, v in job.items() if a != k}], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='nothing to differentiate'):
        KN.tiled_paths_gvjp([{a: v for a, v in job.items() if a not in ('vx', 'vs', 'wu', 'wt')}], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='wt must have shape'):
        KN.tiled_paths_gvjp([dict(job, wt=z(5, 1))], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='Yd must have shape'):
        KN.tiled_paths_gvjp([dict(job, Yd=z(H, 5))], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='gslab must have shape'):
        KN.tiled_paths_gvjp([dict(job, gslab=z(2, bc.numel()))], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='work must have shape'):
        KN.tiled_paths_gvjp([job], bc, 0, H, K, m, work=z(8))


# ---- the public surface ----------------------------------------------------------------------------------------------------------------
M = 37


def _reference(points, wu, wg, wt, params, theta, P, n_sub):
    """per point, on the CPU: n = max(1, ceil((t - T0) / step)) equal steps ending at t, refspec.u_net on the one-path group with
    start = func_h([T0, x]) in the graph of x; autograd in x with its graph, then in theta, of wu u + wg . du/dx + wt ut with
    ut = FL_w . F(t, x, y(t)) from refspec.field at the final state: {key: the gradient summed over the cloud}"""
    from oracle import refspec as R
    T0, T, m = params['T0'], params['T'], params['u_layers']
    th = {k: v.clone().requires_grad_(True) for k, v in theta.items()}
    keys = list(th)
    total = {k: torch.zeros_like(v) for k, v in theta.items()}
    for p, a, b, c in zip(points, wu, wg, wt):
        t = float(p[0])
        x = p[1:].clone().requires_grad_(True)
        n = 0 if t == T0 else max(1, math.ceil((t - T0) / ((T - T0) / n_sub)))
        grid = torch.tensor([T0 + (t - T0) * k / n for k in range(n)] + [t], dtype=F64)
        X = torch.cat((grid.view(1, -1, 1), x.view(1, 1, -1).expand(1, n + 1, -1)), 2)
        s = P.func_h(X[:, 0, :]).reshape(-1)
        ui = R.u_net(th, params, X, s).reshape(-1)[-1]
        gi, = torch.autograd.grad(ui, x, create_graph=True)
        sv = s.detach().view(-1, 1)
        y = torch.relu(torch.relu(sv @ th['IL0_w'].T + th['IL0_b']) @ th['IL2_w'].T + th['IL2_b']) @ th['IL4_w'].T + th['IL4_b']
        xd = x.detach().view(1, -1)
        if n:
            y = R.odeint_fixed(lambda tt, yy: R.field(th, m, xd, tt, yy), y, grid, params['solver'])[:, -1]
        with torch.no_grad():
            assert abs(float((y @ th['FL_w'].T + th['FL_b']).reshape(()) - ui)) <= 1e-14 * max(1.0, abs(float(ui)))   # (the same state)
        ut = (R.field(th, m, xd, grid[-1], y) @ th['FL_w'].T).reshape(())
        J = a * ui + (b * gi).sum() + c * ut
        for k, g in zip(keys, torch.autograd.grad(J, [th[k] for k in keys], allow_unused=True)):
            if g is not None:
                total[k] += g
    return total


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
def test_solver_evaluate_grad_vjp_matches_a_per_point_reference(domain, funcs, method):
    import dataclasses
    P = importlib.import_module('configs.%s_funcs' % funcs)
    S, params = _solver(domain, P, 20, 10, 8, method)
    theta = _theta_of(S, 8)
    pts = _entered_at_T0(domain, params)
    wu, wg, wt = _rand((M,), 31), _rand((M, 3), 32), _rand((M,), 33)
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()[1].copy())
    r = S.evaluate_grad_vjp(pts, wu, wg, wt)
    assert torch.equal(torch.get_rng_state(), rng[0]) and torch.equal(torch.cuda.get_rng_state(), rng[1])
    assert (np.random.get_state()[1] == rng[2]).all()
    assert set(r) == {'u', 'grad', 'ut', 'params'}
    plain = S.evaluate_grad(pts)
    for k in ('u', 'grad', 'ut'):
        assert torch.equal(r[k], plain[k]), k                    # evaluate_grad()'s bits
    worst = {}
    _check_params(S, r, _reference(pts, wu, wg, wt, params, theta, P, params['N_t']), 8, domain, worst)
    print('largest error against the per-point reference, %s %s: %.2e' % (domain, method, max(worst.values())))
    # the module's own entry point, device points, the gradient's weight alone
    rg = S.u_net.module.evaluate_grad_vjp(pts.cuda(), wg=wg.cuda())
    zero = torch.zeros(M, dtype=F64)
    ref_g = _reference(pts, zero, wg, zero, params, theta, P, params['N_t'])
    assert bool((rg['params']['final_linear.bias'] == 0).all()) and bool((ref_g['FL_b'] == 0).all())
    ref_g['FL_b'] = torch.ones(1, dtype=F64)                      # (checked above: exact zeros, no relative comparison)
    rg['params']['final_linear.bias'] = torch.ones(1, dtype=F64, device='cuda')
    _check_params(S, rg, ref_g, 8, domain + ' wg alone')
    # 6. chunks of 16 and 32 paths: the outputs to the bit, the gradient in another order of the slabs' sum
    for chunk in (16, 32):
        S.options = dataclasses.replace(S.options, eval_chunk_paths=chunk)
        rc = S.evaluate_grad_vjp(pts, wu, wg, wt)
        for k in ('u', 'grad', 'ut'):
            assert torch.equal(rc[k], r[k]), k
        for k in r['params']:
            _close(rc['params'][k], r['params'][k], TOL_T, 'chunks of %d %s' % (chunk, k))


def test_evaluate_grad_fn_trains_through_autograd():
    import configs.Ex4_1_funcs as P
    S, params = _solver('Hypercube', P, 20, 10, 8, 'midpoint')
    net = S.u_net.module
    pts = _entered_at_T0('Hypercube', params)
    gen = torch.Generator().manual_seed(41)
    flux = torch.randn(M, 3, dtype=F64, generator=gen).cuda()
    B, c, f = torch.randn(M, 3, dtype=F64, generator=gen).cuda(), 0.7, torch.randn(M, dtype=F64, generator=gen).cuda()
    plist = list(net.parameters())

    def loss_of(r):
        return ((r['ut'] + (B * r['grad']).sum(1) + c * r['u'] - f) ** 2).mean() + ((r['grad'] - flux) ** 2).mean()
    before = S.evaluate_grad(pts)
    r = net.evaluate_grad_fn(pts)
    assert set(r) == {'u', 'grad', 'ut'} and all(v.requires_grad for v in r.values())
    for k in before:
        assert torch.equal(r[k].detach(), before[k]), k
    grads = torch.autograd.grad(loss_of(r), plist)
    # the same cotangents through evaluate_grad_vjp: to the bit
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in r.items()}
    cu, cg, ct = torch.autograd.grad(loss_of(leaf), [leaf['u'], leaf['grad'], leaf['ut']])
    v = net.evaluate_grad_vjp(pts, cu, cg, ct)
    for (name, _), g in zip(net.named_parameters(), grads):
        assert torch.equal(g, v['params'][name]), name
    # ... and the CPU reference
    _check_params(S, v, _reference(pts, cu.cpu(), cg.cpu(), ct.cpu(), params, _theta_of(S, 8), P, params['N_t']), 8, 'residual and flux')
    # a loss of one output alone: the other cotangents are missing
    only = torch.autograd.grad(net.evaluate_grad_fn(pts)['ut'].sum(), plist)
    vt = net.evaluate_grad_vjp(pts, wt=torch.ones(M, dtype=F64))
    for (name, _), g in zip(net.named_parameters(), only):
        assert torch.equal(g, vt['params'][name]), name
    # a few SGD steps on a flux fit lower it; the parameters stay views of the blob
    saved = net.blob.data.clone()
    opt = torch.optim.SGD(net.parameters(), lr=2e-3)
    fit = []
    for _ in range(4):
        opt.zero_grad()
        loss = ((net.evaluate_grad_fn(pts)['grad'] - flux) ** 2).mean()
        loss.backward()
        fit.append(float(loss.detach()))
        opt.step()
        net.blob.check_alias()
    fit.append(float(((S.evaluate_grad(pts)['grad'] - flux) ** 2).mean()))
    print('flux fit under SGD: ' + ' '.join('%.6f' % v for v in fit))
    assert fit[-1] < fit[0] and not torch.equal(net.blob.data, saved)
    # evaluate_grad is bit-reproducible on the updated parameters, and on the restored ones
    a, b = S.evaluate_grad(pts), S.evaluate_grad(pts)
    for k in a:
        assert torch.equal(a[k], b[k]) and not torch.equal(a[k], before[k]), k
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
    w = _rand((M,), 5)
    for name in ('dopri5', 'explicit_adams'):
        S, _ = _solver('Hypercube', P1, 20, 10, 8, name)
        with pytest.raises(XnwanError, match=r'evaluate_grad_vjp\(\).*' + name + '.*fixed-grid'):
            S.evaluate_grad_vjp(pts, w)
        with pytest.raises(XnwanError, match=r'evaluate_grad_vjp\(\).*' + name):
            S.u_net.module.evaluate_grad_fn(pts)
    S, _ = _solver('Hypercube', P1, 20, 10, 8, 'midpoint')
    with pytest.raises(XnwanError, match=r'wu must be None or a tensor \[37\]'):
        S.evaluate_grad_vjp(pts, w.view(M, 1))
    with pytest.raises(XnwanError, match=r'wg must be None or a tensor \[37, 3\]'):
        S.evaluate_grad_vjp(pts, wg=w)
    with pytest.raises(XnwanError, match='at least one of wu'):
        S.evaluate_grad_vjp(pts)
    with pytest.raises(XnwanError, match=r'evaluate_grad_fn\(\): points that require grad'):
        S.u_net.module.evaluate_grad_fn(pts.clone().requires_grad_(True))
    S, _ = _solver('NSphere_THourglass', P3, 20, 10, 8, 'euler')
    from xnode_wan_pde_solver_amd import sampling
    hg = _eval_points('NSphere_THourglass')
    _, at_T0 = sampling.NSphere_THourglass.entry(hg, 1.0, 0, 1)
    first = int((~at_T0).nonzero()[0])
    with pytest.raises(XnwanError, match=r'evaluate_grad_vjp\(\).*entered at T0') as e:
        S.evaluate_grad_vjp(hg, w)
    assert '%d points' % int((~at_T0).sum()) in str(e.value) and 'point %d' % first in str(e.value)
    assert S.evaluate(hg).shape == (M,)      # (evaluate() serves them, as before)
