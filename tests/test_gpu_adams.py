"""Solver 'explicit_adams' on the device (xw_adams_tiled_fwd_multi / _bwd_multi, csrc/xw_tiled.hip): u, Y and the sweep's gx, gs
and summed parameter gradients against the CPU restatement (tests/adams_ref.py) under autograd, for several jobs per launch and
every cotangent form; identical bits run to run and from a captured graph; the module surface u_net(X).backward()."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adams_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
U_ORDER = ['IL0_w', 'IL0_b', 'IL2_w', 'IL2_b', 'IL4_w', 'IL4_b', 'Win', 'Win_b', 'Wh', 'Wh_b', 'Wo', 'Wo_b', 'FL_w', 'FL_b']


def _theta(H, K, m, d, seed):
    from oracle import refspec as R
    torch.manual_seed(seed)
    cfg = {'alpha': 1e8, 'u_layers': m, 'u_hidden_dim': H, 'u_hidden_hidden_dim': K, 'v_layers': 2, 'v_hidden_dim': 8,
           'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'explicit_adams'}
    theta, _ = R.init_parameters(cfg, {'dim': d, 'N_t': 2, 'N_r': 1, 'N_b': 1, 'T0': 0, 'T': 1, 'shape_param': [-1, 1]})
    for k, p in theta.items():               # non-zero biases: every bias path is exercised
        if p.dim() == 1:
            p.copy_(0.3 * torch.randn(p.shape, dtype=F64))
    return theta, torch.cat([theta[k].reshape(-1) for k in U_ORDER])


def _sample(N, L, d, seed):
    """points in the cube, a non-uniform grid that starts off T0 (at 0.25)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(N, d, generator=g) * 2 - 1).double()
    t, _ = torch.sort(torch.rand(L, generator=g).double())
    t = 0.25 + 0.75 * (t - t[0]) / max(float(t[-1] - t[0]), 1e-3) if L > 1 else torch.full((1,), 0.25, dtype=F64)
    start = torch.randn(N, dtype=F64, generator=g)
    ubar = torch.randn(N, L, dtype=F64, generator=g)
    return x, t, start, ubar


def _close(a, b, tol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(float(b.abs().max()), 1e-300)
    err = float((a - b).abs().max()) / scale
    assert err < tol, '%s: max rel-to-scale error %.3e (scale %.3e)' % (what, err, scale)


def _restated(theta, m, x, t, start):
    """the restatement's u [N, L], Y [L, H, N] and the leaves (x, start, parameters) it was computed from"""
    from oracle import refspec as R
    th = {k: v.clone().requires_grad_(True) for k, v in theta.items()}
    x64 = x.clone().requires_grad_(True)
    s = start.clone().requires_grad_(True)
    y0 = torch.relu(torch.relu(s.view(-1, 1) @ th['IL0_w'].T + th['IL0_b']) @ th['IL2_w'].T + th['IL2_b']) @ th['IL4_w'].T + th['IL4_b']
    ys = A.explicit_adams(lambda tt, y: R.field(th, m, x64, tt, y), y0, t)               # [N, L, H]
    u = (ys @ th['FL_w'].T + th['FL_b']).squeeze(2)
    return u, ys.detach().permute(1, 2, 0), [x64, s] + [th[k] for k in U_ORDER]


def _grads(u, leaves, ubar, retain=True):
    gs = torch.autograd.grad((u * ubar).sum(), leaves, retain_graph=retain, allow_unused=True)
    return [g if g is not None else torch.zeros_like(p) for g, p in zip(gs, leaves)]


def _check_grads(gx, gs, flat, want, tol, what):
    if gx is not None:
        _close(gx.t(), want[0], tol, what + ' gx')
        _close(gs, want[1], tol, what + ' gs')
    if flat is not None:
        _close(flat, torch.cat([g.reshape(-1) for g in want[2:]]), tol, what + ' summed parameter gradient')


WIDTHS = [(20, 10, 8), (48, 16, 11), (96, 32, 4), (256, 256, 2), (64, 16, 32)]
CASES = [(0, 1), (0, 13), (1, 2), (1, 32), (2, 3), (2, 13), (3, 4), (3, 32), (4, 13), (4, 3), (0, 32), (2, 4)]


@pytest.mark.parametrize('wi,L', CASES)
def test_forward_and_sweep_match_the_restatement(wi, L):
    """two jobs in one launch (N not a multiple of 16), a stored cotangent, want_x + want_params; every parameter's gradient"""
    from xnode_wan_pde_solver_amd import kernels as KN
    H, K, m = WIDTHS[wi]
    d = (3, 20, 7)[(wi + L) % 3]
    theta, blob = _theta(H, K, m, d, 100 + wi)
    dev = torch.device('cuda')
    bc = blob.to(dev)
    x, t, start, ubar = _sample(203, L, d, 200 + wi + L)
    x2, _, start2, ubar2 = _sample(37, L, d, 300 + wi + L)
    tc = t.to(dev)
    jobs = []
    for x_, s_ in ((x, start), (x2, start2)):
        N = x_.shape[0]
        jobs.append(dict(xT=x_.t().contiguous().to(dev), start=s_.to(dev), u=torch.empty(L, N, dtype=F64, device=dev),
                         Y=torch.empty(L, H, N, dtype=F64, device=dev)))
    KN.adams_tiled_fwd_multi(jobs, tc, bc, H, K, m)
    P = blob.numel()
    outs = []
    for j, ub in zip(jobs, (ubar, ubar2)):
        N = j['xT'].shape[1]
        outs.append(dict(j, ubar=ub.t().contiguous().to(dev), gx=torch.empty(d, N, dtype=F64, device=dev),
                         gs=torch.empty(N, dtype=F64, device=dev), gslab=torch.empty(KN.ode_bwd_slabs(N), P, dtype=F64, device=dev)))
    KN.adams_tiled_bwd_multi(outs, tc, bc, H, K, m, want_x=True, want_params=True)
    for i, (x_, s_, ub) in enumerate(((x, start, ubar), (x2, start2, ubar2))):
        u_ref, Y_ref, leaves = _restated(theta, m, x_, t, s_)
        _close(jobs[i]['u'].t(), u_ref.detach(), 1e-12, 'u job %d' % i)
        _close(jobs[i]['Y'], Y_ref, 1e-12, 'Y job %d' % i)
        want = _grads(u_ref, leaves, ub)
        flat = KN.slab_sum(outs[i]['gslab']).cpu()
        _check_grads(outs[i]['gx'], outs[i]['gs'], flat, want, 1e-10, 'job %d' % i)
        off = 0
        for k, g in zip(U_ORDER, want[2:]):
            n = theta[k].numel()
            _close(flat[off:off + n].view(theta[k].shape), g, 1e-10, 'job %d grad %s' % (i, k))
            off += n


@pytest.mark.parametrize('L', [2, 13])
def test_every_cotangent_form(L):
    """a residual cotangent (boundary form) beside a stored one; the initial-value residual with the all-ones x cotangent; the
    weak form's dI/du; x outputs only; parameter gradients only"""
    from xnode_wan_pde_solver_amd import kernels as KN
    H, K, m, d = 96, 32, 3, 5
    dev = torch.device('cuda')
    theta, blob = _theta(H, K, m, d, 7)
    bc, P = blob.to(dev), blob.numel()
    x, t, start, ubar = _sample(150, L, d, 11)
    x2, _, start2, _ = _sample(45, L, d, 12)
    tc = t.to(dev)
    ja = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), u=torch.empty(L, 150, dtype=F64, device=dev),
              Y=torch.empty(L, H, 150, dtype=F64, device=dev))
    jb = dict(xT=x2.t().contiguous().to(dev), start=start2.to(dev), u=torch.empty(L, 45, dtype=F64, device=dev),
              Y=torch.empty(L, H, 45, dtype=F64, device=dev))
    KN.adams_tiled_fwd_multi([ja, jb], tc, bc, H, K, m)
    ua, Ya, la = _restated(theta, m, x, t, start)
    ub_, Yb, lb = _restated(theta, m, x2, t, start2)
    _close(ja['u'].t(), ua.detach(), 1e-12, 'u a')
    _close(jb['u'].t(), ub_.detach(), 1e-12, 'u b')
    ua_dev, ub_dev = ja['u'].cpu(), jb['u'].cpu()                    # (the residual forms read the device's u)
    mk = lambda N: (torch.empty(d, N, dtype=F64, device=dev), torch.empty(N, dtype=F64, device=dev),   # noqa: E731
                    torch.empty(KN.ode_bwd_slabs(N), P, dtype=F64, device=dev))
    gxa, gsa, sa = mk(150)
    gxb, gsb, sb = mk(45)
    # stored cotangent + boundary residual base + coef (u - ref) in one launch
    ref_b = torch.linspace(-1, 1, 45 * L, dtype=F64).view(L, 45)
    res = dict(u=jb['u'], ref=ref_b.to(dev).contiguous(), coef=0.7, base=0.2, first_only=False)
    KN.adams_tiled_bwd_multi([dict(ja, ubar=ubar.t().contiguous().to(dev), gx=gxa, gs=gsa, gslab=sa),
                              dict(jb, res=res, gx=gxb, gs=gsb, gslab=sb)], tc, bc, H, K, m, want_x=True, want_params=True)
    _check_grads(gxa, gsa, KN.slab_sum(sa).cpu(), _grads(ua, la, ubar), 1e-10, 'stored')
    cot_b = (0.2 + 0.7 * (ub_dev - ref_b)).t()
    _check_grads(gxb, gsb, KN.slab_sum(sb).cpu(), _grads(ub_, lb, cot_b), 1e-10, 'boundary residual')
    # initial-value residual (ubar[0] = base + coef (u[0] - ref), base elsewhere) with the all-ones x cotangent
    ref0 = torch.linspace(0, 1, 150, dtype=F64)
    res0 = dict(u=ja['u'], ref=ref0.to(dev), coef=1.3, base=1.0, first_only=True)
    KN.adams_tiled_bwd_multi([dict(ja, res=res0, gx=gxa, gs=gsa, gslab=sa), dict(jb, gslab=sb, ubar=None)], tc, bc, H, K, m,
                             want_x=True, want_params=True, x_cot_ones=True)
    cot0 = torch.ones(150, L, dtype=F64)
    cot0[:, 0] = 1.0 + 1.3 * (ua_dev[0] - ref0)
    ones = _grads(ua, la, torch.ones(150, L, dtype=F64))
    _check_grads(gxa, gsa, None, ones, 1e-10, 'all-ones x cotangent')
    _check_grads(None, None, KN.slab_sum(sa).cpu(), _grads(ua, la, cot0), 1e-10, 'initial-value residual')
    _check_grads(None, None, KN.slab_sum(sb).cpu(), _grads(ub_, lb, torch.ones(45, L, dtype=F64)), 1e-10, 'no cotangent (ones)')
    # the weak form's dI/du: coef (c + u c') v w (+ base v at the last time index), per-path w
    v = torch.randn(L, 45, dtype=F64, generator=torch.Generator().manual_seed(5))
    w = torch.rand(45, dtype=F64, generator=torch.Generator().manual_seed(6))
    c, cp = torch.randn(L, 45, dtype=F64), torch.randn(L, 45, dtype=F64)
    resw = dict(u=jb['u'], ref=v.to(dev), coef=0.4, base=0.3, weak=dict(w=w.to(dev), c=c.to(dev), cp=cp.to(dev)))
    KN.adams_tiled_bwd_multi([dict(jb, res=resw, gx=gxb, gs=gsb, gslab=sb)], tc, bc, H, K, m, want_x=True, want_params=True)
    cotw = 0.4 * (c + ub_dev * cp) * v * w.view(1, -1)
    cotw[L - 1] += 0.3 * v[L - 1]
    _check_grads(gxb, gsb, KN.slab_sum(sb).cpu(), _grads(ub_, lb, cotw.t()), 1e-10, 'weak form')
    # x outputs only / parameter gradients only
    KN.adams_tiled_bwd_multi([dict(ja, ubar=ubar.t().contiguous().to(dev), gx=gxa, gs=gsa)], tc, bc, H, K, m, want_x=True,
                             want_params=False)
    _check_grads(gxa, gsa, None, _grads(ua, la, ubar), 1e-10, 'x only')
    KN.adams_tiled_bwd_multi([dict(ja, ubar=ubar.t().contiguous().to(dev), gslab=sa)], tc, bc, H, K, m, want_x=False,
                             want_params=True)
    _check_grads(None, None, KN.slab_sum(sa).cpu(), _grads(ua, la, ubar, retain=False), 1e-10, 'parameters only')


@pytest.mark.parametrize('L', [2, 3])
@pytest.mark.parametrize('N', [17, 1])
@pytest.mark.parametrize('d,H,K,m', [(2, 5, 3, 1), (4, 33, 17, 2)])
def test_startup_steps_are_the_rk4_stepper_to_the_bit(d, H, K, m, N, L):
    """With two or three sample times 'explicit_adams' consists of rk4 start-up steps only (no history term reaches a step: fbar
    is an exact zero).  The forward passes run the same step function; the sweeps hold two texts of the rk4 reverse and the tail
    (kt_ode_bwd's own, and the shared ones of csrc/xw_tiled_blocks.h), which this test pins to each other: u, Y and the sweep's
    gx, gs, gslab are the rk4 stepper's bits -- x only, parameters only, both.  N = 17: a full tile and a tile of one path;
    (4, 33, 17, 2) crosses the padding to 16 rows and 4 columns."""
    from xnode_wan_pde_solver_amd import kernels as KN
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 40 + H)
    bc, P = blob.to(dev), blob.numel()
    x, t, start, ubar = _sample(N, L, d, 50 + N + L)
    tc, ub = t.to(dev), ubar.t().contiguous().to(dev)

    def fwd_job():
        return dict(xT=x.t().contiguous().to(dev), start=start.to(dev), u=torch.full((L, N), float('nan'), dtype=F64, device=dev),
                    Y=torch.full((L, H, N), float('nan'), dtype=F64, device=dev))

    rk, ab = fwd_job(), fwd_job()
    KN.tiled_ode_fwd_multi([rk], tc, bc, KN.METHODS['rk4'], H, K, m)
    KN.adams_tiled_fwd_multi([ab], tc, bc, H, K, m)
    assert torch.isfinite(rk['Y']).all()
    assert torch.equal(ab['u'], rk['u']) and torch.equal(ab['Y'], rk['Y'])
    for want_x, want_params in ((True, False), (False, True), (True, True)):
        outs = []
        for sweep in (lambda jobs, **kw: KN.tiled_ode_bwd_multi(jobs, tc, bc, KN.METHODS['rk4'], H, K, m, **kw),
                      lambda jobs, **kw: KN.adams_tiled_bwd_multi(jobs, tc, bc, H, K, m, **kw)):
            o = dict(rk, ubar=ub)
            if want_x:
                o.update(gx=torch.full((d, N), float('nan'), dtype=F64, device=dev), gs=torch.full((N,), float('nan'), dtype=F64, device=dev))
            if want_params:
                o.update(gslab=torch.full((KN.ode_bwd_slabs(N), P), float('nan'), dtype=F64, device=dev))
            sweep([o], want_x=want_x, want_params=want_params)
            outs.append(o)
        for k in (('gx', 'gs') if want_x else ()) + (('gslab',) if want_params else ()):
            assert torch.isfinite(outs[0][k]).all(), k
            assert torch.equal(outs[1][k], outs[0][k]), '%s (want_x %s, want_params %s)' % (k, want_x, want_params)


def test_results_are_bitwise_reproducible_and_graph_replayable():
    from xnode_wan_pde_solver_amd import kernels as KN
    H, K, m, d, L, N = 64, 16, 5, 7, 13, 500
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 3)
    bc = blob.to(dev)
    x, t, start, ubar = _sample(N, L, d, 5)
    a = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), u=torch.empty(L, N, dtype=F64, device=dev),
             Y=torch.empty(L, H, N, dtype=F64, device=dev))
    tc, ub = t.to(dev), ubar.t().contiguous().to(dev)
    gx, gs = torch.empty(d, N, dtype=F64, device=dev), torch.empty(N, dtype=F64, device=dev)
    slab = torch.empty(KN.ode_bwd_slabs(N), blob.numel(), dtype=F64, device=dev)

    def launch():
        KN.tiled_ode_fwd_multi([a], tc, bc, KN.ADAMS, H, K, m)
        KN.tiled_ode_bwd_multi([dict(a, ubar=ub, gx=gx, gs=gs, gslab=slab)], tc, bc, KN.ADAMS, H, K, m, want_x=True, want_params=True)

    def run():
        launch()
        return [a['u'].clone(), a['Y'].clone(), gx.clone(), gs.clone(), slab.clone()]

    first, second = run(), run()
    for x_, y_ in zip(first, second):
        assert torch.equal(x_, y_)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for v in (a['u'], a['Y'], gx, gs, slab):
        v.fill_(float('nan'))
    with torch.cuda.graph(g):
        launch()
    g.replay()
    torch.cuda.synchronize()
    for x_, y_ in zip(first, [a['u'], a['Y'], gx, gs, slab]):
        assert torch.equal(x_, y_)


def test_refusals_on_the_device_path():
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    H, K, m, d, L, N = 20, 10, 8, 3, 5, 20
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 1)
    bc = blob.to(dev)
    x, t, start, ubar = _sample(N, L, d, 2)
    a = dict(xT=x.t().contiguous().to(dev), start=start.to(dev), u=torch.empty(L, N, dtype=F64, device=dev),
             Y=torch.empty(L, H, N, dtype=F64, device=dev))
    KN.adams_tiled_fwd_multi([a], t.to(dev), bc, H, K, m)
    gx, gs = torch.empty(d, N, dtype=F64, device=dev), torch.empty(N, dtype=F64, device=dev)
    with pytest.raises(XnwanError, match="'explicit_adams' with adjoint=True"):
        KN.adams_tiled_bwd_multi([dict(a, ubar=ubar.t().contiguous().to(dev), gx=gx, gs=gs)], t.to(dev), bc, H, K, m, want_x=True,
                                 want_params=False, adjoint=True)
    # the fused containers do not run it: a status code, not a launch
    with pytest.raises(XnwanError, match='XW_E_ARG'):
        KN.ode_fwd(a['xT'], t.to(dev), a['start'], bc, KN.ADAMS, H, K, m)


# ---- the module surface ------------------------------------------------------------------------------------------------------
def _module_solver(domain='Hypercube'):
    import configs.Ex4_1_funcs as P
    from src.training import NODE_WAN_solver
    params = {'alpha': 1e3, 'u_layers': 8, 'u_hidden_dim': 20, 'u_hidden_hidden_dim': 10, 'v_layers': 4, 'v_hidden_dim': 50,
              'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'explicit_adams',
              'dim': 4, 'N_t': 8, 'N_r': 60, 'N_b': 30, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 1, 'domain': domain}
    torch.manual_seed(13)
    return NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, torch.device('cuda'), './',
                           func_u_sol=P.func_u_sol, p=2), params


def _theta_of(S):
    """the oracle's parameter dict from the solver's u_net (reference names: the `module.` prefix of PathParallel)"""
    from oracle import refspec as R
    named = dict(S.u_net.named_parameters())
    return {k: named[n].detach().cpu().double().clone().requires_grad_(True) for n, k in R.u_names(S.u_net.module.num_layers)}


def test_module_forward_and_backward_match_the_restatement():
    """u_net(X).sum().backward() with solver 'explicit_adams' at (20, 10, 8) on the cube: u, d/dX and every parameter's gradient"""
    import configs.Ex4_1_funcs as P
    from oracle import refspec as R
    S, params = _module_solver()
    net = S.u_net.module
    assert net.family == 'tiled' and net.kdims == (20, 10) and S.engine.stepper == 'tiled'
    assert 'explicit_adams' in S.plan()['ode_solver'] and 'tiled' in S.plan()['stepper']
    g = torch.Generator().manual_seed(3)
    N, L = 77, 9
    X = torch.empty(N, L, 5, dtype=torch.float32)
    X[:, :, 1:] = (torch.rand(N, 1, 4, generator=g) * 2 - 1).float()
    X[:, :, 0] = torch.linspace(0, 1, L).view(1, -1)
    Xg = X.clone().requires_grad_(True)
    out = S.u_net(Xg)
    out.sum().backward()
    th = _theta_of(S)
    Xr = X.clone().requires_grad_(True)
    u_ref = A.u_net(th, params, Xr, P.func_h(Xr[:, 0, :]))
    u_ref.sum().backward()
    _close(out.squeeze(2), u_ref.detach(), 1e-12, 'u')
    _close(Xg.grad[:, 0, 1:], Xr.grad[:, 0, 1:], 1e-9, 'dX')
    named = dict(S.u_net.named_parameters())
    for n_, k_ in R.u_names(net.num_layers):
        _close(named[n_].grad, th[k_].grad, 1e-10, 'grad ' + k_)


def test_evaluation_path_over_a_bound_pad_grid():
    """paths that start neither at T0 nor on the boundary: integrated from T0 over domain.bound_pad's densified grid (fillt)"""
    import configs.Ex4_1_funcs as P
    S, params = _module_solver()
    net = S.u_net.module
    g = torch.Generator().manual_seed(8)
    N = 40
    X = torch.empty(N, 3, 5, dtype=torch.float32)
    X[:, :, 1:] = (torch.rand(N, 1, 4, generator=g) * 1.6 - 0.8).float()
    X[:, :, 0] = torch.tensor([0.33, 0.61, 0.97]).view(1, -1)
    Xg = X.clone().requires_grad_(True)
    out = S.u_net(Xg)
    out.sum().backward()
    assert out.shape == (N, 3, 1)
    _, gather, filled = S.domain(params['shape_param'], params['dim'], 0, 1, params['N_t']).bound_pad(X)
    assert filled.shape[0] > 4                                          # (AB steps past the rk4 start-up)
    th = _theta_of(S)
    Xr = X.clone().requires_grad_(True)
    padded = Xr[:, :1, :].repeat(1, filled.shape[0], 1)
    padded[:, :, 0] = filled.view(1, -1).to(padded.dtype)
    start = P.func_g(Xr[:, 0, :].unsqueeze(1)).reshape(-1).double()
    u_ref = A.u_net(th, params, padded, start)[:, gather.long()]
    u_ref.sum().backward()
    _close(out.squeeze(2), u_ref.detach(), 1e-12, 'u')
    _close(Xg.grad[:, 0, 1:], Xr.grad[:, 0, 1:], 1e-9, 'dX')
    from oracle import refspec as R
    named = dict(S.u_net.named_parameters())
    for n_, k_ in R.u_names(net.num_layers):
        _close(named[n_].grad, th[k_].grad, 1e-10, 'grad ' + k_)
