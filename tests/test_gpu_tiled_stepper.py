"""The tiled stepper family (csrc/xw_tiled.hip) on the device: forward u, Y and the sweep's gx, gs and summed parameter gradient
against the oracle's torch restatement and its autograd, at widths neither of the other two families serves; agreement with the
generic path where both run; identical bits run to run and from a captured graph."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F64 = torch.float64
U_ORDER = ['IL0_w', 'IL0_b', 'IL2_w', 'IL2_b', 'IL4_w', 'IL4_b', 'Win', 'Win_b', 'Wh', 'Wh_b', 'Wo', 'Wo_b', 'FL_w', 'FL_b']


def _cfg(H, K, m, solver):
    return {'alpha': 1e8, 'u_layers': m, 'u_hidden_dim': H, 'u_hidden_hidden_dim': K, 'v_layers': 2, 'v_hidden_dim': 8,
            'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': solver}


def _theta(H, K, m, d, seed):
    from oracle import refspec as R
    torch.manual_seed(seed)
    theta, _ = R.init_parameters(_cfg(H, K, m, 'rk4'), {'dim': d, 'N_t': 2, 'N_r': 1, 'N_b': 1, 'T0': 0, 'T': 1,
                                                         'shape_param': [-1, 1]})
    for k, p in theta.items():               # non-zero biases: every bias path is exercised
        if p.dim() == 1:
            p.copy_(0.3 * torch.randn(p.shape, dtype=F64))
    blob = torch.cat([theta[k].reshape(-1) for k in U_ORDER])
    return theta, blob


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


def _oracle(theta, H, K, m, solver, x, t, start, ubar):
    """u [N, L], Y [L, H, N] and the gradients of <ubar, u> w.r.t. x, start and every parameter (autograd)"""
    from oracle import refspec as R
    th = {k: v.clone().requires_grad_(True) for k, v in theta.items()}
    x64 = x.clone().requires_grad_(True)
    s = start.clone().requires_grad_(True)
    y0 = torch.relu(torch.relu(s.view(-1, 1) @ th['IL0_w'].T + th['IL0_b']) @ th['IL2_w'].T + th['IL2_b']) @ th['IL4_w'].T + th['IL4_b']
    ys = R.odeint_fixed(lambda tt, y: R.field(th, m, x64, tt, y), y0, t, solver)          # [N, L, H]
    u = (ys @ th['FL_w'].T + th['FL_b']).squeeze(2)
    grads = torch.autograd.grad((u * ubar).sum(), [x64, s] + [th[k] for k in U_ORDER], allow_unused=True)
    grads = [g if g is not None else torch.zeros_like(p) for g, p in zip(grads, [x64, s] + [th[k] for k in U_ORDER])]
    return u.detach(), ys.detach().permute(1, 2, 0), grads


WIDTHS = [(65, 16, 1), (20, 17, 2), (96, 32, 8), (128, 64, 10), (256, 128, 4)]
DS, LS = (3, 20, 100), (2, 9, 33)


@pytest.mark.parametrize('solver', ['euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize('wi', range(len(WIDTHS)))
def test_tiled_forward_and_sweep_match_the_oracle(wi, solver):
    from xnode_wan_pde_solver_amd import kernels as KN
    H, K, m = WIDTHS[wi]
    si = ['euler', 'midpoint', 'rk4'].index(solver)
    d, L, N = DS[(wi + si) % 3], LS[(wi + 2 * si) % 3], 1000
    assert KN.stepper_family(H, K, m) == 'tiled'
    theta, blob = _theta(H, K, m, d, 100 + wi)
    x, t, start, ubar = _sample(N, L, d, 200 + wi + 7 * si)
    u_ref, Y_ref, grads = _oracle(theta, H, K, m, solver, x, t, start, ubar)
    dev = torch.device('cuda')
    xT, tc, sc, bc = x.t().contiguous().to(dev), t.to(dev), start.to(dev), blob.to(dev)
    mid = KN.method_id(solver)
    u, Y = KN.tiled_ode_fwd(xT, tc, sc, bc, mid, H, K, m)
    _close(u.t(), u_ref, 1e-12, 'u')
    _close(Y, Y_ref, 1e-12, 'Y')
    gx, gs, slab = KN.tiled_ode_bwd(xT, tc, sc, bc, Y, ubar.t().contiguous().to(dev), mid, H, K, m, want_x=True, want_params=True)
    assert slab.shape == (KN.ode_bwd_slabs(N), KN.theta_size(d, H, K))
    _close(gx.t(), grads[0], 1e-10, 'gx')
    _close(gs, grads[1], 1e-10, 'gs')
    flat, off = KN.slab_sum(slab).cpu(), 0
    for k, g in zip(U_ORDER, grads[2:]):
        n = theta[k].numel()
        _close(flat[off:off + n].view(theta[k].shape), g, 1e-10, 'grad ' + k)
        off += n
    _close(flat, torch.cat([g.reshape(-1) for g in grads[2:]]), 1e-10, 'summed parameter gradient')


def _jobs(N, L, d, H, seed, dev):
    x, t, start, ubar = _sample(N, L, d, seed)
    return dict(xT=x.t().contiguous().to(dev), start=start.to(dev), u=torch.empty(L, N, dtype=F64, device=dev),
                Y=torch.empty(L, H, N, dtype=F64, device=dev)), t.to(dev), ubar.t().contiguous().to(dev)


@pytest.mark.parametrize('solver', ['euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize('H,K,m', [(64, 16, 12), (48, 16, 11)])
def test_tiled_and_generic_families_agree(H, K, m, solver):
    """where the generic path serves, both families compute the same values (to rounding) under every launch form the engine
    uses: two jobs in one launch, a stored cotangent, residual cotangents formed inside the sweep, the all-ones x cotangent"""
    from xnode_wan_pde_solver_amd import kernels as KN
    d, L = 5, 9
    assert KN.stepper_family(H, K, m) == 'generic' and KN.stepper_family(H, K, m, 'generic') == 'tiled'
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 7)
    bc = blob.to(dev)
    mid = KN.method_id(solver)
    a, t, ubar = _jobs(300, L, d, H, 11, dev)
    b, _, _ = _jobs(37, L, d, H, 12, dev)
    outs = {}
    for fam in ('generic', 'tiled'):
        ja, jb = dict(a, u=torch.empty_like(a['u']), Y=torch.empty_like(a['Y'])), dict(b, u=torch.empty_like(b['u']), Y=torch.empty_like(b['Y']))
        fwd = KN.tiled_ode_fwd_multi if fam == 'tiled' else KN.ode_fwd_multi
        bwd = KN.tiled_ode_bwd_multi if fam == 'tiled' else KN.ode_bwd_multi
        fwd([ja, jb], t, bc, mid, H, K, m)
        o = [ja['u'], ja['Y'], jb['u'], jb['Y']]
        P = blob.numel()
        # stored cotangent + residual (boundary form) in one launch, x and parameters
        sa = torch.empty(KN.ode_bwd_slabs(300), P, dtype=F64, device=dev)
        sb = torch.empty(KN.ode_bwd_slabs(37), P, dtype=F64, device=dev)
        gxa, gsa = torch.empty(d, 300, dtype=F64, device=dev), torch.empty(300, dtype=F64, device=dev)
        gxb, gsb = torch.empty(d, 37, dtype=F64, device=dev), torch.empty(37, dtype=F64, device=dev)
        res = dict(u=jb['u'], ref=torch.linspace(-1, 1, 37 * L, dtype=F64, device=dev).view(L, 37).contiguous(), coef=0.7, base=0.2,
                   first_only=False)
        bwd([dict(ja, ubar=ubar, gx=gxa, gs=gsa, gslab=sa), dict(jb, res=res, gx=gxb, gs=gsb, gslab=sb)], t, bc, mid, H, K, m,
            want_x=True, want_params=True)
        o += [gxa, gsa, KN.slab_sum(sa), gxb, gsb, KN.slab_sum(sb)]
        # the all-ones x cotangent beside the initial-value residual (ubar == base at every l >= 1), second job without x outputs
        res0 = dict(u=ja['u'], ref=torch.linspace(0, 1, 300, dtype=F64, device=dev), coef=1.3, base=1.0, first_only=True)
        bwd([dict(ja, res=res0, gx=gxa, gs=gsa, gslab=sa), dict(jb, gslab=sb)], t, bc, mid, H, K, m, want_x=True, want_params=True,
            x_cot_ones=True)
        o += [gxa.clone(), gsa.clone(), KN.slab_sum(sa), KN.slab_sum(sb)]
        # x outputs only
        bwd([dict(ja, ubar=ubar, gx=gxa, gs=gsa)], t, bc, mid, H, K, m, want_x=True, want_params=False)
        o += [gxa.clone(), gsa.clone()]
        outs[fam] = [v.clone() for v in o]
    for i, (g_, t_) in enumerate(zip(outs['generic'], outs['tiled'])):
        _close(t_, g_, 1e-12, 'output %d' % i)


def test_tiled_results_are_bitwise_reproducible_and_graph_replayable():
    from xnode_wan_pde_solver_amd import kernels as KN
    H, K, m, d, L, N = 96, 32, 5, 7, 9, 500
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 3)
    bc = blob.to(dev)
    a, t, ubar = _jobs(N, L, d, H, 5, dev)
    P = blob.numel()
    gx, gs = torch.empty(d, N, dtype=F64, device=dev), torch.empty(N, dtype=F64, device=dev)
    slab = torch.empty(KN.ode_bwd_slabs(N), P, dtype=F64, device=dev)

    def run():
        KN.tiled_ode_fwd_multi([a], t, bc, 2, H, K, m)
        KN.tiled_ode_bwd_multi([dict(a, ubar=ubar, gx=gx, gs=gs, gslab=slab)], t, bc, 2, H, K, m, want_x=True, want_params=True)
        return [a['u'].clone(), a['Y'].clone(), gx.clone(), gs.clone(), slab.clone()]

    first, second = run(), run()
    for x_, y_ in zip(first, second):
        assert torch.equal(x_, y_)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                   # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for v in (a['u'], a['Y'], gx, gs, slab):
        v.fill_(float('nan'))
    with torch.cuda.graph(g):
        KN.tiled_ode_fwd_multi([a], t, bc, 2, H, K, m)
        KN.tiled_ode_bwd_multi([dict(a, ubar=ubar, gx=gx, gs=gs, gslab=slab)], t, bc, 2, H, K, m, want_x=True, want_params=True)
    g.replay()
    torch.cuda.synchronize()
    for x_, y_ in zip(first, [a['u'], a['Y'], gx, gs, slab]):
        assert torch.equal(x_, y_)


def test_tiled_refusals():
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    H, K, m, d, L, N = 128, 32, 2, 3, 3, 20
    dev = torch.device('cuda')
    _, blob = _theta(H, K, m, d, 1)
    bc = blob.to(dev)
    a, t, ubar = _jobs(N, L, d, H, 2, dev)
    KN.tiled_ode_fwd_multi([a], t, bc, 1, H, K, m)
    gx, gs = torch.empty(d, N, dtype=F64, device=dev), torch.empty(N, dtype=F64, device=dev)
    with pytest.raises(XnwanError, match='adjoint'):
        KN.tiled_ode_bwd_multi([dict(a, ubar=ubar, gx=gx, gs=gs)], t, bc, 1, H, K, m, want_x=True, want_params=False, adjoint=True)
    with pytest.raises(XnwanError, match='fixed-grid'):
        KN.tiled_ode_fwd_multi([a], t, bc, KN.DOPRI5, H, K, m)
    # the fused and generic entry points keep refusing these widths
    with pytest.raises(XnwanError):
        KN.ode_fwd(a['xT'], t, a['start'], bc, 1, H, K, m)
