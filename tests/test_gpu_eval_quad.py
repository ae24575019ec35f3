"""Second-order forward jets over a ragged group (csrc/xw_tiled_paths_jet.hip: kt_paths_jet2) and the quadratic forms, the diffusion
term and the strong-form residual at scattered points built on them (kernels.tiled_paths_jet, evalpaths.evaluate_points_quad /
evaluate_points_lap / evaluate_points_residual, evaluate_quad / evaluate_lap of XNODE and NODE_WAN_solver, evaluate_residual of
NODE_WAN_solver) on the device.

Kernel level, inside the guard-banded, poisoned arena of tests/guarded.py (the workspace handed in through work=), at the shapes of
tests/test_gpu_eval_paths.py (its _ragged: a path without a step beside one with L - 1 in one tile; m = 1 puts the tanh's curvature
on the first pre-activation; H = 65 has a ragged last row block; N = 17 and 37 a ragged last tile; L = 1 no step anywhere), R = 3
directions at N = 1 and N = 37 (3 x 3 blocks) and R = 1 elsewhere, random directions with a fixed seed, qs nonzero:
 (a) every path and direction against oracle.refspec run on that path ALONE (tests/test_gpu_eval_hess.py::_oracle_alone, direction 0
     the very case that file computes): ju, and quu against vx . hx + vs hs + gs qs -- relative to scale below that file's
     TOL_G = 1e-10, the project's bound for this block arithmetic;
 (b) a path without a step has quu == 0 exactly where qs == 0, else quu == gs qs and ju == gs vs to 1e-12;
 (c) every output element written, no guard element touched, theta and the inputs bit-unchanged;
 (d) the same bits with and without the nstep hint, under a permutation of the paths, under a permutation of the directions and with
     one direction launched alone as R = 1, with qs NULL against zeros, with each of ju and quu asked for alone, from a
     captured-graph replay;
 (e) u bit-equal to tiled_paths_fwd's, and (2 vx, 2 vs, 4 qs) gives 2 ju and 4 quu to the bit.
Public surface: evaluate_quad, evaluate_lap and evaluate_residual on the cube, the cone and the hourglass's T0-entered points against
autograd's Hessian of x -> refspec.u_net([[T0, x] ... [t, x]], h([T0, x])) per point on the CPU (tests/test_gpu_eval_hess.py::
_reference), computed once per network and cloud."""
import dataclasses
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402
from test_gpu_tiled_stepper import F64, _close, _theta  # noqa: E402
from test_gpu_eval_paths import LS, METHODS, NETS, NS, _eval_points, _ragged, _solver, _theta_of  # noqa: E402
from test_gpu_eval_hess import TOL_G, _directions, _oracle_alone, _reference as _hess_reference  # noqa: E402

pytestmark = pytest.mark.gpu

OUTS = ('ju', 'quu')
INPUTS = ('xT', 'start', 'tT', 'nstep')


def _general_funcs():
    spec = importlib.util.spec_from_file_location('general_funcs', os.path.join(os.path.dirname(__file__), 'golden', 'general_funcs.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _curves(N, d, R, seed):
    """vx [R, N, d], vs [R, N], qs [R, N]: direction 0 is _directions(N, d, seed + 2), what tests/test_gpu_eval_hess.py uses"""
    dirs = [_directions(N, d, seed + 2 + 100 * r) for r in range(R)]
    qs = torch.randn(R, N, generator=torch.Generator().manual_seed(seed + 7), dtype=F64)
    return torch.stack([v for v, _ in dirs]), torch.stack([s for _, s in dirs]), qs


def _jet(KN, arena, blob, inp, vx, vs, qs, H, K, m, mid, hint=True, want=('u',) + OUTS):
    """one guarded launch on the inputs `inp` (views of the arena) with the curves vx [R, d, N], vs [R, N], qs [R, N] or None (views
    too): the job with the outputs asked for and its guarded workspace"""
    d, N = inp['xT'].shape
    R = vx.shape[0]
    job = {k: inp[k] for k in ('xT', 'start', 'tT')}
    if hint:
        job['nstep'] = inp['nstep']
    job.update(vx=vx, vs=vs)
    if qs is not None:
        job['qs'] = qs
    for k in want:
        job[k] = arena.out(*((N,) if k == 'u' else (R, N)), name=k)
    work = arena.out(KN.lib.xw_paths_tiled_jet_work(d, H, K, m) * R * ((N + 15) // 16), name='jet_work')
    KN.tiled_paths_jet([job], blob, mid, H, K, m, work=work)
    return job


def _inputs(arena, x, start, tT, n):
    return dict(xT=arena.inp(x.t(), name='xT'), start=arena.inp(start, name='start'), tT=arena.inp(tT, name='tT'),
                nstep=n.to(torch.int32).to(arena.device))


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('net', range(len(NETS)))
@pytest.mark.parametrize('method', METHODS)
def test_per_path_jet(method, net, N):
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m = NETS[net]
    R = 3 if N in (1, 37) else 1
    mid = KN.method_id(method)
    theta, blob_h = _theta(H, K, m, d, 300 + net)
    dev = torch.device('cuda')
    worst = 0.0
    for L in LS:
        seed = 1000 * net + 10 * N + L
        x, start, n, tT = _ragged(N, L, d, seed)
        vx, vs, qs = _curves(N, d, R, seed)
        if L == 5 and N > 1:
            assert int(n[0]) == 0 and int(n[1]) == 4                 # no step beside four, in one tile
        assert float(qs.abs().min()) > 0
        arena = G.Arena(dev)
        with arena.workspaces(KN):
            blob = arena.inp(blob_h, name='theta')
            inp = _inputs(arena, x, start, tT, n)
            vxd, vsd, qsd = arena.inp(vx.transpose(1, 2), name='vx'), arena.inp(vs, name='vs'), arena.inp(qs, name='qs')
            zero = arena.inp(torch.zeros(R, N, dtype=F64), name='qs0')
            torch.cuda.synchronize()
            kept = {k: inp[k].clone() for k in INPUTS}
            kept.update(theta=blob.clone(), vx=vxd.clone(), vs=vsd.clone(), qs=qsd.clone(), zero=zero.clone())
            fj = dict(inp, u=arena.out(L, N, name='u_fwd'), Y=arena.out(L, H, N, name='Y'))
            KN.tiled_paths_fwd([fj], blob, mid, H, K, m)
            gs = arena.out(N, name='gs')
            KN.tiled_paths_grad([dict({k: fj[k] for k in INPUTS + ('Y',)}, gs=gs)], blob, mid, H, K, m)
            plain = _jet(KN, arena, blob, inp, vxd, vsd, qsd, H, K, m, mid, hint=False)
            hinted = _jet(KN, arena, blob, inp, vxd, vsd, qsd, H, K, m, mid)
            alone = {k: _jet(KN, arena, blob, inp, vxd, vsd, qsd, H, K, m, mid, want=(k,)) for k in OUTS}
            qzero = _jet(KN, arena, blob, inp, vxd, vsd, zero, H, K, m, mid)
            qnull = _jet(KN, arena, blob, inp, vxd, vsd, None, H, K, m, mid)
            gen = torch.Generator().manual_seed(seed + 1)
            perm = torch.randperm(N, generator=gen)
            moved = _jet(KN, arena, blob, _inputs(arena, x[perm], start[perm], tT[:, perm].contiguous(), n[perm]),
                         arena.inp(vx[:, perm].transpose(1, 2), name='vx'), arena.inp(vs[:, perm], name='vs'),
                         arena.inp(qs[:, perm], name='qs'), H, K, m, mid)
            dperm = torch.randperm(R, generator=gen)
            turned = _jet(KN, arena, blob, inp, arena.inp(vx[dperm].transpose(1, 2), name='vx'), arena.inp(vs[dperm], name='vs'),
                          arena.inp(qs[dperm], name='qs'), H, K, m, mid)
            r1 = R - 1
            single = _jet(KN, arena, blob, inp, arena.inp(vx[r1:r1 + 1].transpose(1, 2), name='vx'), arena.inp(vs[r1:r1 + 1], name='vs'),
                          arena.inp(qs[r1:r1 + 1], name='qs'), H, K, m, mid)
            scaled = _jet(KN, arena, blob, inp, arena.inp(2 * vx.transpose(1, 2), name='vx'), arena.inp(2 * vs, name='vs'),
                          arena.inp(4 * qs, name='qs'), H, K, m, mid)
        # (c) every output element written, no guard element touched; theta and the inputs unchanged
        jobs = [plain, hinted, qzero, qnull, moved, turned, single, scaled] + list(alone.values())
        arena.check(written=[j[k] for j in jobs for k in ('u',) + OUTS if k in j] + [fj['u'], fj['Y'], gs])
        what = '%s %s N %d L %d R %d' % (method, NETS[net], N, L, R)
        for k in INPUTS:
            assert torch.equal(inp[k], kept[k]), '%s changed: %s' % (k, what)
        assert torch.equal(blob, kept['theta']) and torch.equal(vxd, kept['vx']) and torch.equal(vsd, kept['vs']), what
        assert torch.equal(qsd, kept['qs']) and torch.equal(zero, kept['zero']), what
        # (a) every path and direction against the oracle on that path alone
        ju_ref, quu_ref, gs_ref = torch.empty(R, N, dtype=F64), torch.empty(R, N, dtype=F64), None
        for r in range(R):
            key = (method, net, N, L) if r == 0 else (method, net, N, L, 'jet', r)
            ju_r, hx_r, hs_r, _, gs_ref = _oracle_alone(theta, H, K, m, method, x, start, n, tT, vx[r], vs[r], key)
            ju_ref[r], quu_ref[r] = ju_r, (vx[r].t() * hx_r).sum(0) + vs[r] * hs_r + gs_ref * qs[r]
        for k, ref in (('ju', ju_ref), ('quu', quu_ref)):
            scale = float(ref.abs().max())
            err = float((plain[k].cpu() - ref).abs().max()) / scale
            worst = max(worst, err)
            print('%s %s: rel-to-scale error %.3e (scale %.3e)' % (k, what, err, scale))
        assert float(ju_ref.abs().max()) > 0 and float(quu_ref.abs().max()) > 0            # (not a comparison of zeros)
        _close(plain['ju'], ju_ref, TOL_G, 'ju ' + what)
        _close(plain['quu'], quu_ref, TOL_G, 'quu ' + what)
        if L > 1:                                                    # ... and the curvature itself, without the qs term
            bare = quu_ref - gs_ref.view(1, N) * qs
            assert float(bare.abs().max()) > 0
            _close(qzero['quu'], bare, TOL_G, 'quu with qs = 0 ' + what)
        # (b) no step: no curvature, and both orders are the lift's alone
        still = n.to(dev) == 0
        assert bool((qzero['quu'][:, still] == 0).all()), 'no step, qs == 0: quu == 0 exactly: ' + what
        if bool(still.any()):
            for k, c in (('ju', vsd), ('quu', qsd)):
                want = (gs.view(1, N) * c)[:, still]
                assert float((plain[k][:, still] - want).abs().max()) <= 1e-12 * float(want.abs().max()), '%s without a step: %s' % (k, what)
        _close(gs, gs_ref, TOL_G, 'gs ' + what)
        # (d) the same bits with the hint, each output alone, beside other neighbours, in another block of the grid, qs NULL
        pd, dd = perm.to(dev), dperm.to(dev)
        for k in OUTS:
            assert torch.equal(hinted[k], plain[k]), 'nstep %s %s' % (k, what)
            assert torch.equal(alone[k][k], plain[k]), 'alone %s %s' % (k, what)
            assert torch.equal(moved[k], plain[k][:, pd]), 'permuted paths %s %s' % (k, what)
            assert torch.equal(turned[k], plain[k][dd]), 'permuted directions %s %s' % (k, what)
            assert torch.equal(single[k], plain[k][r1:r1 + 1]), 'one direction alone %s %s' % (k, what)
            assert torch.equal(qnull[k], qzero[k]), 'qs NULL %s %s' % (k, what)
        assert torch.equal(qzero['ju'], plain['ju']), 'ju does not see qs: ' + what
        # (e) u: the forward's bits, from every launch; scaling by a power of two is exact
        for j, tag in ((plain, 'plain'), (hinted, 'nstep'), (qnull, 'qs NULL'), (turned, 'directions'), (single, 'R = 1'), (scaled, 'scaled')):
            assert torch.equal(j['u'], fj['u'][L - 1]), 'u %s %s' % (tag, what)
        assert torch.equal(moved['u'], fj['u'][L - 1][pd]), 'u permuted ' + what
        assert torch.equal(scaled['ju'], 2 * plain['ju']) and torch.equal(scaled['quu'], 4 * plain['quu']), 'scaling ' + what
    print('largest rel-to-scale error of %s %s N %d: %.3e' % (method, NETS[net], N, worst))


def test_graph_replay_gives_the_same_bits():
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m = NETS[2]
    N, L, R = 37, 5, 3
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 7)
    x, start, n, tT = _ragged(N, L, d, 8)
    vx, vs, qs = _curves(N, d, R, 9)
    bc = blob.to(dev)
    new = lambda *s: torch.empty(*s, dtype=F64, device=dev)      # noqa: E731
    job = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), tT=tT.to(dev), nstep=n.to(torch.int32).to(dev),
               vx=vx.transpose(1, 2).contiguous().to(dev), vs=vs.to(dev), qs=qs.to(dev))
    first = dict(u=new(N), ju=new(R, N), quu=new(R, N))
    KN.tiled_paths_jet([dict(job, **first)], bc, 2, H, K, m)
    full = dict(job, **{k: torch.empty_like(v) for k, v in first.items()})
    work = KN.paths_jet_work(d, H, K, m, R * ((N + 15) // 16), dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        KN.tiled_paths_jet([full], bc, 2, H, K, m, work=work)        # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in first:
        full[k].fill_(float('nan'))
    with torch.cuda.graph(g):
        KN.tiled_paths_jet([full], bc, 2, H, K, m, work=work)
    g.replay()
    torch.cuda.synchronize()
    for k in first:
        assert torch.equal(full[k], first[k]), k


def test_kernel_wrapper_refusals():
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    d, H, K, m = NETS[0]
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 1)
    bc = blob.to(dev)
    x, start, n, tT = _ragged(5, 3, d, 2)
    z = lambda *s: torch.zeros(*s, dtype=F64, device=dev)         # noqa: E731
    job = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), tT=tT.to(dev), vx=z(2, d, 5), vs=z(2, 5), quu=z(2, 5))
    for mid in (KN.DOPRI5, KN.ADAMS):
        with pytest.raises(XnwanError, match='fixed-grid'):
            KN.tiled_paths_jet([job], bc, mid, H, K, m)
    with pytest.raises(XnwanError, match='nstep'):
        KN.tiled_paths_jet([dict(job, nstep=n.to(dev))], bc, 0, H, K, m)                           # (int64: the kernel reads int32)
    for k in ('vx', 'vs'):
        with pytest.raises(XnwanError, match=k + r' is needed'):
            KN.tiled_paths_jet([{q: v for q, v in job.items() if q != k}], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='no output'):
        KN.tiled_paths_jet([{k: v for k, v in job.items() if k != 'quu'}], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match=r'vx must be a tensor \[R, d, N\]'):
        KN.tiled_paths_jet([dict(job, vx=z(d, 5))], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='vx must have shape'):
        KN.tiled_paths_jet([dict(job, vx=z(2, 5, d))], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='qs must have shape'):
        KN.tiled_paths_jet([dict(job, qs=z(5))], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='u must have shape'):
        KN.tiled_paths_jet([dict(job, u=z(2, 5))], bc, 0, H, K, m)
    with pytest.raises(XnwanError, match='work must have shape'):
        KN.tiled_paths_jet([job], bc, 0, H, K, m, work=z(7))


# ---- the public surface ----------------------------------------------------------------------------------------------------------------
_REFERENCE = {}


def _reference(pts, params, theta, P, n_sub, key):
    """(u, grad, hess) of tests/test_gpu_eval_hess.py::_reference, once per (cloud, resolution): the networks of _solver are drawn
    from one seed, so the cases of a domain share it; the key carries a digest of theta all the same"""
    key = (key, n_sub, pts.shape[0], tuple(round(float(v.double().sum()), 12) for v in theta.values()))
    if key not in _REFERENCE:
        _REFERENCE[key] = _hess_reference(pts, params, theta, P, n_sub)
    return _REFERENCE[key]


def _table(fa, pts):
    M, d = pts.shape[0], pts.shape[1] - 1
    X = pts.view(M, 1, 1 + d)
    return torch.stack([torch.stack([fa(X, i, j).double().reshape(M) for j in range(d)], 1) for i in range(d)], 1)


def _check_surface(S, pts, params, theta, P, what):
    GF = _general_funcs()
    M, d, R = pts.shape[0], pts.shape[1] - 1, 4
    V = torch.randn(M, R, d, generator=torch.Generator().manual_seed(43), dtype=F64)
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()[1].copy())
    q = S.evaluate_quad(pts, V)
    lp = S.evaluate_lap(pts)
    assert torch.equal(torch.get_rng_state(), rng[0]) and torch.equal(torch.cuda.get_rng_state(), rng[1])
    assert (np.random.get_state()[1] == rng[2]).all()
    assert set(q) == {'u', 'dv', 'quad'} and set(lp) == {'u', 'lap'}
    assert q['u'].shape == (M,) and q['dv'].shape == (M, R) and q['quad'].shape == (M, R) and lp['lap'].shape == (M,)
    assert all(t.dtype == F64 and t.is_cuda and not t.requires_grad and t.is_contiguous() for t in list(q.values()) + list(lp.values()))
    u = S.evaluate(pts)
    assert torch.equal(q['u'], u) and torch.equal(lp['u'], u), what                     # evaluate's bits
    u_ref, g_ref, h_ref = _reference(pts, params, theta, P, params['N_t'], what)
    assert float(h_ref.abs().max()) > 0
    _close(q['u'], u_ref, 1e-12, 'u ' + what)
    _close(q['quad'], torch.einsum('mri,mij,mrj->mr', V, h_ref, V), TOL_G, 'quad ' + what)
    _close(q['dv'], torch.einsum('mi,mri->mr', g_ref, V), TOL_G, 'dv ' + what)
    trace = torch.diagonal(h_ref, dim1=1, dim2=2).sum(1)
    _close(lp['lap'], trace, TOL_G, 'lap ' + what)
    hs = S.evaluate_hess(pts)
    _close(lp['lap'], hs['lap'], TOL_G, 'lap against evaluate_hess ' + what)
    print('%s: lap against evaluate_hess %.3e of its scale' % (what, float((lp['lap'] - hs['lap']).abs().max() / hs['lap'].abs().max())))
    # a coefficient: one matrix, a diagonal table, a general table per point
    const = _table(GF.const_a, pts[:1])[0]
    for name, a in (('const_a', const), ('diag_a', _table(GF.diag_a, pts)), ('func_a', _table(GF.func_a, pts))):
        got = S.evaluate_lap(pts, a)
        _close(got['lap'], (a * h_ref).sum((-2, -1)), TOL_G, 'lap %s %s' % (name, what))
        assert torch.equal(got['u'], u)
    _close(S.evaluate_lap(pts, torch.eye(d, dtype=F64))['lap'], trace, TOL_G, 'lap identity ' + what)
    assert torch.equal(S.evaluate_lap(pts, torch.eye(d, dtype=F64))['lap'], lp['lap'])
    # another resolution, device input, the module's own entry points; chunks of 16 paths: the same bits
    r5 = S.u_net.module.evaluate_quad(pts.cuda(), V.cuda(), n_sub=5)
    _close(r5['quad'], torch.einsum('mri,mij,mrj->mr', V, _reference(pts, params, theta, P, 5, what)[2], V), TOL_G, 'quad n_sub 5 ' + what)
    assert torch.equal(S.u_net.module.evaluate_lap(pts)['lap'], lp['lap'])
    general = S.evaluate_lap(pts, _table(GF.func_a, pts))
    chunked = dataclasses.replace(S.options, eval_chunk_paths=16)
    keep, S.options = S.options, chunked
    try:
        for k, t in S.evaluate_quad(pts, V).items():
            assert torch.equal(t, q[k]), k
        for k, t in S.evaluate_lap(pts).items():
            assert torch.equal(t, lp[k]), k
        for k, t in S.evaluate_lap(pts, _table(GF.func_a, pts)).items():
            assert torch.equal(t, general[k]), k
    finally:
        S.options = keep
    # an empty cloud
    e = S.evaluate_quad(pts[:0], V[:0])
    assert e['quad'].shape == (0, R) and e['dv'].shape == (0, R) and e['u'].shape == (0,) and e['quad'].is_cuda
    assert S.evaluate_lap(pts[:0])['lap'].shape == (0,)


@pytest.mark.parametrize('domain,funcs,method', [('Hypercube', 'Ex4_1', 'midpoint'), ('NSphere_TCone', 'Ex4_3', 'rk4')])
def test_solver_evaluate_quad_and_lap_on_the_cube_and_the_cone(domain, funcs, method):
    from xnode_wan_pde_solver_amd._lib import XnwanError
    P = importlib.import_module('configs.%s_funcs' % funcs)
    S, params = _solver(domain, P, method=method)
    pts = _eval_points(domain)
    assert int((pts[:, 0] == 0).sum()) > 0                          # a point at t = T0: no step
    _check_surface(S, pts, params, _theta_of(S, 8), P, domain)
    for V in (torch.zeros(37, 3, dtype=F64), torch.zeros(37, 2, 4, dtype=F64), torch.zeros(36, 2, 3, dtype=F64),
              torch.zeros(37, 0, 3, dtype=F64), [[0.0] * 3] * 37):
        with pytest.raises(XnwanError, match=r'evaluate_quad\(\): V must be a tensor \[M, R, d\] = \[37, R, 3\]'):
            S.evaluate_quad(pts, V)
    for a in (torch.zeros(3, dtype=F64), torch.zeros(3, 4, dtype=F64), torch.zeros(36, 3, 3, dtype=F64), 'identity'):
        with pytest.raises(XnwanError, match=r'evaluate_lap\(\): a must be None .* \[d, d\] = \[3, 3\] or \[M, d, d\] = \[37, 3, 3\]'):
            S.evaluate_lap(pts, a)
    with pytest.raises(XnwanError, match=r'evaluate_lap\(\).*\[M, 4\]'):
        S.evaluate_lap(pts[:, :3])
    if domain == 'Hypercube':
        early = pts.clone()
        early[9, 0] = -0.25
        for call, who in ((lambda: S.evaluate_quad(early, torch.zeros(37, 1, 3, dtype=F64)), 'quad'), (lambda: S.evaluate_lap(early), 'lap'),
                          (lambda: S.evaluate_residual(early), 'residual')):
            with pytest.raises(XnwanError, match=r'evaluate_%s\(\).*t >= t_in' % who) as e:
                call()
            assert '1 points' in str(e.value) and 'point 9' in str(e.value)


def test_solver_evaluate_quad_and_lap_on_the_hourglass():
    """the points entered at T0 are served; the cloud with its re-entered points is refused, with the count and the first index"""
    import configs.Ex4_3_funcs as P
    from xnode_wan_pde_solver_amd import sampling
    from xnode_wan_pde_solver_amd._lib import XnwanError
    S, params = _solver('NSphere_THourglass', P, method='euler')
    pts = _eval_points('NSphere_THourglass')
    _, at_T0 = sampling.NSphere_THourglass.entry(pts, 1.0, 0, 1)
    late = (~at_T0).nonzero().view(-1)
    assert 0 < late.numel() < 37
    _check_surface(S, pts[at_T0].contiguous(), params, _theta_of(S, 8), P, 'hourglass')
    for call in (lambda: S.evaluate_quad(pts, torch.zeros(37, 2, 3, dtype=F64)), lambda: S.evaluate_lap(pts), lambda: S.evaluate_residual(pts)):
        with pytest.raises(XnwanError, match='entered at T0') as e:
            call()
        assert '%d points' % late.numel() in str(e.value) and 'point %d,' % int(late[0]) in str(e.value)


def _general_div_a(X, j):
    """the closed form of sum_i d_i a_ij for tests/golden/general_funcs.py::func_a"""
    x1, x2 = X[..., 1], X[..., 2]
    return x1 * (1.0 if j == 0 else 0.1 * torch.cos(x2)) + (1.0 + 0.5 * x1 ** 2) * (0.0 if j == 1 else -0.1 * torch.sin(x2))


@pytest.mark.parametrize('name', ['Ex4_1', 'v1', 'const', 'diag'])
def test_solver_evaluate_residual_on_the_cube(name):
    import configs.Ex4_1_funcs as E
    GF = _general_funcs()
    fa, fb, fc = (E.func_a, E.func_b, E.func_c) if name == 'Ex4_1' else GF.variant(name)
    P = types.SimpleNamespace(func_a=fa, func_b=fb, func_c=fc, func_h=E.func_h, func_f=E.func_f, func_g=E.func_g, func_u_sol=E.func_u_sol)
    S, params = _solver('Hypercube', P, method='midpoint')
    pts = _eval_points('Hypercube')
    M, d = pts.shape[0], 3
    r = S.evaluate_residual(pts)
    assert set(r) == {'u', 'ut', 'grad', 'diffusion', 'residual'}
    assert all(t.dtype == F64 and t.is_cuda and not t.requires_grad for t in r.values())
    assert r['residual'].shape == (M,) and r['diffusion'].shape == (M,) and r['grad'].shape == (M, d)
    g = S.evaluate_grad(pts)
    for k in ('u', 'grad', 'ut'):
        assert torch.equal(r[k], g[k]), k                              # evaluate_grad's bits
    _, _, h_ref = _reference(pts, params, _theta_of(S, 8), P, params['N_t'], 'Hypercube')
    u, ut, grad = g['u'].cpu(), g['ut'].cpu(), g['grad'].cpu()
    X = pts.view(M, 1, 1 + d)
    A = _table(fa, pts)
    B = torch.stack([fb(X, i).double().reshape(M) for i in range(d)], 1)
    if name == 'v1':
        D = torch.stack([_general_div_a(X, j).reshape(M) for j in range(d)], 1)
    elif name == 'diag':
        D = torch.stack([0.6 * pts[:, 1 + j] for j in range(d)], 1)    # a_jj = 1 + 0.3 x_j^2
    else:
        D = torch.zeros(M, d, dtype=F64)
    c = fc(X, u.view(M, 1, 1)).double().reshape(M)
    f = E.func_f(X).double().reshape(M)
    terms = dict(ut=ut, diffusion=(A * h_ref).sum((1, 2)), diva=(D * grad).sum(1), adv=(B * grad).sum(1), react=c * u, f=f)
    want = terms['ut'] - terms['diffusion'] - terms['diva'] + terms['adv'] + terms['react'] - terms['f']
    scale = max(float(t.abs().max()) for t in terms.values())
    err_d = float((r['diffusion'].cpu() - terms['diffusion']).abs().max())
    err_r = float((r['residual'].cpu() - want).abs().max())
    print('%s: diffusion error %.3e, residual error %.3e, largest term %.3e' % (name, err_d, err_r, scale))
    assert scale > 0 and float(terms['diffusion'].abs().max()) > 0
    assert err_d <= TOL_G * scale and err_r <= TOL_G * scale, name
    if name in ('v1', 'diag'):
        assert float(terms['diva'].abs().max()) > 0
    # a callable div a gives what autograd through func_a gives
    by_hand = {'v1': _general_div_a, 'diag': lambda X, j: 0.6 * X[..., 1 + j]}.get(name, lambda X, j: torch.zeros(X.shape[:-1], dtype=X.dtype))
    r2 = S.evaluate_residual(pts, div_a=by_hand)
    assert float((r2['residual'] - r['residual']).abs().max()) <= 1e-13 * scale, name
    assert torch.equal(r2['diffusion'], r['diffusion'])
    # device input: the callables (h among them) then run on the device, whose sin, cos and exp differ from the host's in the last
    # bits -- every term within a few ulp of its own size, so the sum within 1e-12 of the largest term; an empty cloud
    rd = S.evaluate_residual(pts.cuda())
    assert float((rd['residual'] - r['residual']).abs().max()) <= 1e-12 * scale, name
    assert S.evaluate_residual(pts[:0])['residual'].shape == (0,)


@pytest.mark.parametrize('solver', ['dopri5', 'explicit_adams'])
def test_solvers_without_a_fixed_grid_are_refused(solver):
    import configs.Ex4_1_funcs as P
    from xnode_wan_pde_solver_amd._lib import XnwanError
    S, _ = _solver('Hypercube', P, method=solver)
    pts = _eval_points('Hypercube')
    for who, call in (('quad', lambda: S.evaluate_quad(pts, torch.zeros(37, 2, 3, dtype=F64))), ('lap', lambda: S.evaluate_lap(pts)),
                      ('residual', lambda: S.evaluate_residual(pts))):
        with pytest.raises(XnwanError, match=r'evaluate_%s\(\): solver %r is not served' % (who, solver)):
            call()


def test_a_domain_class_without_entry_is_refused():
    import configs.Ex4_1_funcs as P
    from xnode_wan_pde_solver_amd._lib import XnwanError
    S, _ = _solver('Hypercube', P)

    class Slab:
        pass
    S.u_net.module.domain = Slab
    pts = _eval_points('Hypercube')
    for who, call in (('quad', lambda: S.evaluate_quad(pts, torch.zeros(37, 2, 3, dtype=F64))), ('lap', lambda: S.evaluate_lap(pts)),
                      ('residual', lambda: S.evaluate_residual(pts))):
        with pytest.raises(XnwanError, match=r'evaluate_%s\(\): the domain class Slab has no entry' % who):
            call()
    with pytest.raises(XnwanError, match=r"evaluate_residual\(\): div_a must be 'autograd' or a callable"):
        S.evaluate_residual(pts, div_a='closed-form')
