"""solver 'dopri5' on the MI355X (csrc/xw_dopri.hip through kernels.dopri5_fwd / dopri5_sweep and the XNODE autograd surface)
against the CPU restatement tests/dopri5_ref.py: the same step decisions, grids, outputs and gradients."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dopri5_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu
F64 = torch.float64
U_ORDER = ['IL0_w', 'IL0_b', 'IL2_w', 'IL2_b', 'IL4_w', 'IL4_b', 'Win', 'Win_b', 'Wh', 'Wh_b', 'Wo', 'Wo_b', 'FL_w', 'FL_b']


def _case(d, H, K, m, N, L, seed):
    from oracle import refspec as R
    cfg = {'alpha': 1e8, 'u_layers': m, 'u_hidden_dim': H, 'u_hidden_hidden_dim': K, 'v_layers': 9, 'v_hidden_dim': 50, 'n1': 2,
           'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'dopri5'}
    torch.manual_seed(seed)
    theta, _ = R.init_parameters(cfg, {'dim': d, 'N_t': L, 'N_r': 1, 'N_b': 1, 'T0': 0, 'T': 1, 'shape_param': [-1, 1]})
    for p in theta.values():
        if p.dim() == 1:
            p.copy_(0.3 * torch.randn(p.shape, dtype=F64))
    g = torch.Generator().manual_seed(seed + 1)
    x = (torch.rand(N, d, generator=g) * 2 - 1).float()
    t, _ = torch.sort(torch.rand(L, generator=g).float())
    t[0], t[-1] = 0.0, 1.0
    X = torch.cat((t.view(1, L, 1).expand(N, L, 1), x.view(N, 1, d).expand(N, L, d)), 2).contiguous()
    start = torch.randn(N, dtype=F64, generator=g)
    return cfg, theta, X, start


def _blob(theta, d, H, K, m):
    """theta in the kernels' layout at the width of its container (nets.Blob: narrower networks embedded, zero-padded)"""
    from xnode_wan_pde_solver_amd import kernels as KN, nets
    Hc, Kc = KN.ode_container(H, K, m)
    slots, total = nets._u_slots(d, H, K, Hc, Kc, m > 1)
    blob = torch.zeros(total, dtype=F64)
    keys = [k for k in U_ORDER if m > 1 or k not in ('Wh', 'Wh_b')]
    for k, (off, r, c, ld) in zip(keys, slots):
        p = theta[k].reshape(r, c)
        for i in range(r):
            blob[off + i * ld:off + i * ld + c] = p[i]
    return blob.cuda(), Hc, Kc


def _gpu_fwd(theta, X, start, d, H, K, m, want_Y=True, **kw):
    from xnode_wan_pde_solver_amd import kernels as KN
    blob, Hc, Kc = _blob(theta, d, H, K, m)
    N, L = X.shape[0], X.shape[1]
    xT = X[:, 0, 1:].double().t().contiguous().cuda()
    t = X[0, :, 0].double().contiguous().cuda()
    s = start.cuda()
    u = torch.full((L, N), float('nan'), dtype=F64, device='cuda')
    Y = torch.full((L, Hc, N), float('nan'), dtype=F64, device='cuda') if want_Y else None
    rec, = KN.dopri5_fwd([dict(xT=xT, start=s, u=u, Y=Y)], t, blob, Hc, Kc, m, H, **kw)
    return dict(u=u, Y=Y, rec=rec, xT=xT, t=t, s=s, blob=blob, Hc=Hc, Kc=Kc)


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _ref_Y(theta, cfg, X, start, frozen=None):
    from oracle import refspec as R
    m = cfg['u_layers']
    s = start.reshape(-1, 1)
    y0 = torch.relu(torch.relu(s @ theta['IL0_w'].T + theta['IL0_b']) @ theta['IL2_w'].T + theta['IL2_b']) @ theta['IL4_w'].T \
        + theta['IL4_b']
    x64 = X[:, 0, 1:].double()
    ys, info = D.dopri5(lambda t, y: R.field(theta, m, x64, t, y), y0, X[0, :, 0], count=y0.numel(), frozen=frozen)
    return ys, info


# The step-size sequence is a smooth function of the rounding only when the field is: with ReLU layers in it (u_layers >= 2) the
# error estimate's sensitivity to the state is large near the kinks and 1e-16 differences grow over the steps -- the restatement
# on its own takes 63 or 65 attempts for the first case below depending on torch's thread count.  So the step decisions are
# pinned exactly on tanh-only fields (u_layers = 1; the lift's ReLUs act once), and the ReLU fields against the restatement
# integrated on the device's own accepted grid.  The error estimate is a sum of terms ~1e4 times larger than itself, so its
# rounding (and the device tanh's last bits) moves the ratio by up to ~1e-9 relative (one path: few terms), the step sizes by a
# fifth of that: measured 5e-12 (37 paths) and 1.9e-10 (one path); the grids are compared at 1e-9.
GRID_TOL = 1e-9
SMOOTH_CASES = [(3, 12, 6, 1, 37, 5, 1), (20, 20, 10, 1, 37, 6, 2), (3, 32, 12, 1, 37, 4, 3), (20, 32, 12, 1, 1, 5, 4),
                (3, 20, 10, 1, 4096, 6, 5), (20, 12, 6, 1, 1, 3, 6), (20, 32, 12, 1, 4096, 5, 7)]
RELU_CASES = [(3, 12, 6, 8, 37, 5, 1), (20, 20, 10, 8, 37, 6, 2), (3, 32, 12, 10, 37, 4, 3), (20, 32, 12, 8, 1, 5, 4),
              (3, 20, 10, 10, 4096, 6, 5), (20, 12, 6, 10, 1, 3, 6)]


def _grid_of(info):
    return torch.tensor([info['steps'][0][0]] + [a + b for a, b in info['steps']], dtype=F64)


@pytest.mark.parametrize('d,H,K,m,N,L,seed', SMOOTH_CASES)
def test_forward_against_the_restatement(d, H, K, m, N, L, seed):
    cfg, theta, X, start = _case(d, H, K, m, N, L, seed)
    ys, info = _ref_Y(theta, cfg, X, start)
    assert info['gap'] > 1e-9, 'bad fixture: a step decision within %.1e of the threshold' % info['gap']
    u_ref = (ys @ theta['FL_w'].T + theta['FL_b']).squeeze(2)
    g = _gpu_fwd(theta, X, start, d, H, K, m)
    rec = g['rec']
    assert (rec.n_att, rec.n_acc) == (info['n_att'], info['n_acc'])
    assert _rel(rec.grid, _grid_of(info)) < GRID_TOL
    assert _rel(g['u'].t(), u_ref) < 1e-9
    assert _rel(g['Y'][:, :H, :].permute(2, 0, 1), ys) < 1e-9
    if g['Hc'] > H:
        assert float(g['Y'][:, H:, :].abs().max()) == 0.0                 # the padding units stay exactly zero


@pytest.mark.parametrize('d,H,K,m,N,L,seed', RELU_CASES)
def test_forward_relu_field_on_its_own_grid(d, H, K, m, N, L, seed):
    cfg, theta, X, start = _case(d, H, K, m, N, L, seed)
    g = _gpu_fwd(theta, X, start, d, H, K, m)
    rec = g['rec']
    ys, _ = _ref_Y(theta, cfg, X, start, frozen=rec.steps)
    assert _rel(g['u'].t(), (ys @ theta['FL_w'].T + theta['FL_b']).squeeze(2)) < 1e-9
    assert _rel(g['Y'][:, :H, :].permute(2, 0, 1), ys) < 1e-9
    # ... and both solves are within tolerance of each other
    ys2, info = _ref_Y(theta, cfg, X, start)
    assert _rel(g['Y'][:, :H, :].permute(2, 0, 1), ys2) < 1e-4
    assert abs(rec.n_acc - info['n_acc']) <= max(3, info['n_acc'] // 5) and rec.n_att >= rec.n_acc


def test_two_jobs_with_their_own_controllers():
    """two jobs in one launch that need different numbers of steps: each equals the same job run alone (to the bit) and the
    restatement (tanh field: the step decisions too)"""
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m, L = 5, 20, 10, 1, 6
    cfg, theta, X1, s1 = _case(d, H, K, m, 40, L, 21)
    _, _, X2, s2 = _case(d, H, K, m, 70, L, 22)
    X2 = X2.clone()
    X2[:, :, 0] = X1[0, :, 0].view(1, L)                                    # (the jobs of a launch share t)
    s2 = 100.0 * s2                                                         # a larger start: 9 attempts, 7 accepted (8, 8)
    blob, Hc, Kc = _blob(theta, d, H, K, m)
    t = X1[0, :, 0].double().cuda()
    jobs = [dict(xT=X[:, 0, 1:].double().t().contiguous().cuda(), start=s.cuda(), u=torch.empty(L, X.shape[0], dtype=F64, device='cuda'))
            for X, s in ((X1, s1), (X2, s2))]
    recs = KN.dopri5_fwd(jobs, t, blob, Hc, Kc, m, H)
    assert (recs[0].n_att, recs[0].n_acc) != (recs[1].n_att, recs[1].n_acc)
    for rec, (X, s), j in zip(recs, ((X1, s1), (X2, s2)), jobs):
        _, info = _ref_Y(theta, cfg, X, s)
        assert (rec.n_att, rec.n_acc) == (info['n_att'], info['n_acc'])
        assert _rel(rec.grid, _grid_of(info)) < GRID_TOL
        alone = _gpu_fwd(theta, X, s, d, H, K, m, want_Y=False)
        assert torch.equal(alone['u'], j['u']) and torch.equal(alone['rec'].grid, rec.grid)


def _ref_grads(theta, cfg, X, start, cot, frozen):
    th = {k: v.clone().requires_grad_(True) for k, v in theta.items()}
    x64 = X[:, 0, 1:].double().clone().requires_grad_(True)
    s = start.clone().requires_grad_(True)
    N, L = X.shape[0], X.shape[1]
    Xd = torch.cat((X[:, :, :1].double(), x64.view(N, 1, -1).expand(N, L, -1)), 2)
    u, _ = D.u_net(th, cfg, Xd, s, frozen=frozen)
    keys = [k for k in U_ORDER if k in th]
    gs = torch.autograd.grad(cot(u), [x64, s] + [th[k] for k in keys], allow_unused=True)
    return u.detach(), gs[0], gs[1], {k: (g if g is not None else torch.zeros_like(th[k])) for k, g in zip(keys, gs[2:])}


@pytest.mark.parametrize('d,H,K,m,N,L,seed', [(4, 20, 10, 8, 37, 5, 31), (3, 12, 6, 2, 20, 4, 32), (6, 32, 12, 10, 19, 3, 33)])
@pytest.mark.parametrize('form', ['ubar', 'ones_x', 'res', 'res_first', 'weak'])
def test_sweep_against_frozen_grid_autograd(d, H, K, m, N, L, seed, form):
    from xnode_wan_pde_solver_amd import kernels as KN
    cfg, theta, X, start = _case(d, H, K, m, N, L, seed)
    g = _gpu_fwd(theta, X, start, d, H, K, m, want_Y=False)
    gen = torch.Generator().manual_seed(seed + 7)
    ubar = torch.randn(N, L, dtype=F64, generator=gen)
    ref = torch.randn(N, L, dtype=F64, generator=gen)
    w = torch.rand(N, dtype=F64, generator=gen)
    job = dict(xT=g['xT'], start=g['s'], rec=g['rec'])
    u_dev = g['u']
    if form in ('ubar', 'ones_x'):
        if form == 'ones_x':
            ubar[:, 1:] = 1.0
        cot = lambda u: (u * ubar).sum()                                   # noqa: E731
        job['ubar'] = ubar.t().contiguous().cuda()
    elif form == 'res':                                                     # base + coef (u - ref) at every time
        cot = lambda u: (0.3 * u + 0.35 * (u - ref) ** 2).sum()            # noqa: E731
        job['res'] = dict(u=u_dev, ref=ref.t().contiguous().cuda(), coef=0.7, base=0.3, first_only=False)
    elif form == 'res_first':                                               # base + coef (u - ref) at t_0 only
        cot = lambda u: (0.3 * u).sum() + 0.35 * ((u[:, 0] - ref[:, 0]) ** 2).sum()   # noqa: E731
        job['res'] = dict(u=u_dev, ref=ref[:, 0].contiguous().cuda(), coef=0.7, base=0.3, first_only=True)
    else:                                                                   # coef d(kappa u^2)/du v w + base v at l = L-1
        cot = lambda u: (0.4 * 0.5 * u ** 2 * ref * w.view(-1, 1)).sum() + 0.2 * (u[:, -1] * ref[:, -1]).sum()   # noqa: E731
        job['res'] = dict(u=u_dev, ref=ref.t().contiguous().cuda(), coef=0.4, base=0.2,
                          weak=dict(w=w.cuda(), ckappa=0.5))
    _, gx_r, gs_r, gp_r = _ref_grads(theta, cfg, X, start, cot, g['rec'].steps)
    P = KN.theta_size(d, g['Hc'], g['Kc'])
    job.update(gx=torch.empty(d, N, dtype=F64, device='cuda'), gs=torch.empty(N, dtype=F64, device='cuda'),
               gslab=torch.empty(KN.ode_bwd_slabs(N), P, dtype=F64, device='cuda'))
    ones = form == 'ones_x'
    KN.dopri5_sweep([job], g['t'], g['blob'], g['Hc'], g['Kc'], m, want_x=True, want_params=True, x_cot_ones=ones)
    flat = KN.slab_sum(job['gslab']).cpu()
    # the parameter gradients, at the network's own widths
    from xnode_wan_pde_solver_amd import nets
    slots, _ = nets._u_slots(d, H, K, g['Hc'], g['Kc'], m > 1)
    keys = [k for k in U_ORDER if m > 1 or k not in ('Wh', 'Wh_b')]
    for k, (off, r, c, ld) in zip(keys, slots):
        got = torch.stack([flat[off + i * ld:off + i * ld + c] for i in range(r)]).reshape(gp_r[k].shape)
        assert _rel(got, gp_r[k]) < 1e-9, (form, k, _rel(got, gp_r[k]))
    if ones:                                                                # x-side outputs of the all-ones cotangent
        _, gx_r, gs_r, _ = _ref_grads(theta, cfg, X, start, lambda u: u.sum(), g['rec'].steps)
    assert _rel(job['gx'].t(), gx_r) < 1e-9, form
    assert _rel(job['gs'], gs_r) < 1e-9, form


def test_record_growth_gives_the_same_results():
    d, H, K, m, N, L = 4, 20, 10, 8, 50, 5
    cfg, theta, X, start = _case(d, H, K, m, N, L, 41)
    a = _gpu_fwd(theta, X, start, d, H, K, m, rtol=1e-10, atol=1e-12, cap=2, chunk=3)
    b = _gpu_fwd(theta, X, start, d, H, K, m, rtol=1e-10, atol=1e-12, cap=4000)
    assert a['rec'].n_acc > 20 and a['rec'].cap > 2
    assert torch.equal(a['u'], b['u']) and torch.equal(a['Y'], b['Y']) and torch.equal(a['rec'].grid, b['rec'].grid)
    assert a['rec'].n_att == b['rec'].n_att


def test_step_limit_raises():
    from xnode_wan_pde_solver_amd._lib import XnwanError
    d, H, K, m, N, L = 4, 20, 10, 8, 16, 4
    cfg, theta, X, start = _case(d, H, K, m, N, L, 51)
    with pytest.raises(XnwanError, match='step limit of 3 accepted steps'):
        _gpu_fwd(theta, X, start, d, H, K, m, max_steps=3)


def test_autograd_surface_and_determinism():
    """u_net(X).sum().backward() with solver 'dopri5' against the restatement's frozen-grid autograd; twice, bit-identical"""
    from xnode_wan_pde_solver_amd import nets
    d, H, K, m, N, L = 4, 20, 10, 8, 96, 8
    cfg, theta, X, start = _case(d, H, K, m, N, L, 61)
    setup = {'dim': d, 'T0': 0, 'T': 1}
    h = lambda Z: start.view(-1, 1).to(Z.device)                            # noqa: E731  (the start values of this sample)
    net = nets.XNODE(H, 1, h, None, setup, K, m, None, solver='dopri5')
    named = dict(net.named_parameters())
    from oracle import refspec as R
    with torch.no_grad():
        for name, key in R.u_names(m):
            named[name[len('module.'):]].copy_(theta[key].reshape(named[name[len('module.'):]].shape))
    net.bind(torch.device('cuda'))
    runs = []
    for _ in range(2):
        net.zero_grad()
        Xc = X.cuda().requires_grad_(True)
        u = net(Xc, starts_at_T0=True)
        u.sum().backward()
        runs.append((u.detach().clone(), Xc.grad.clone(), [p.grad.clone() for p in net.parameters()]))
    u_r, gx_r, _, gp_r = _ref_grads(theta, cfg, X, start, lambda u: u.sum(), net.last_dopri5.steps)
    assert _rel(runs[0][0].squeeze(2), u_r) < 1e-9
    assert _rel(runs[0][1][:, 0, 1:], gx_r) < 1e-6                         # (X is float32, the reference's cube sample: so is its gradient)
    for (name, key), p in zip(R.u_names(m), net.parameters()):
        assert _rel(p.grad, gp_r[key].reshape(p.shape)) < 1e-9, name
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
