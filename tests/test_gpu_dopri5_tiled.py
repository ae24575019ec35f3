"""solver 'dopri5' on the tiled stepper family on the MI355X (csrc/xw_tdopri.hip through kernels.dopri5_fwd / dopri5_sweep with
stepper='tiled', and the XNODE autograd surface with dopri5_stepper = 'tiled') against the CPU restatement tests/dopri5_ref.py and
against the vector implementation (csrc/xw_dopri.hip) at the widths both serve.

Tolerances are those of tests/test_gpu_dopri5.py, with the reasoning given there: 1e-9 relative-to-scale for u, Y and every
gradient against the restatement, GRID_TOL = 1e-9 for the accepted grids, 1e-6 for the float32 sample's x gradient."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_dopri5 import (_case, _ref_Y, _ref_grads, _grid_of, _rel, GRID_TOL, SMOOTH_CASES, U_ORDER)  # noqa: E402

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _blob(theta, d, H, K, m):
    """theta in the kernels' layout at the widths the network binds at: its container (narrower networks embedded, zero-padded)
    or, beyond the containers, its own"""
    from xnode_wan_pde_solver_amd import kernels as KN, nets
    Hc, Kc = KN.stepper_kdims(H, K, m)
    slots, total = nets._u_slots(d, H, K, Hc, Kc, m > 1)
    blob = torch.zeros(total, dtype=F64)
    keys = [k for k in U_ORDER if m > 1 or k not in ('Wh', 'Wh_b')]
    for k, (off, r, c, ld) in zip(keys, slots):
        p = theta[k].reshape(r, c)
        for i in range(r):
            blob[off + i * ld:off + i * ld + c] = p[i]
    return blob.cuda(), Hc, Kc


def _gpu_fwd(theta, X, start, d, H, K, m, want_Y=True, stepper='tiled', **kw):
    from xnode_wan_pde_solver_amd import kernels as KN
    blob, Hc, Kc = _blob(theta, d, H, K, m)
    N, L = X.shape[0], X.shape[1]
    xT = X[:, 0, 1:].double().t().contiguous().cuda()
    t = X[0, :, 0].double().contiguous().cuda()
    s = start.cuda()
    u = torch.full((L, N), float('nan'), dtype=F64, device='cuda')
    Y = torch.full((L, Hc, N), float('nan'), dtype=F64, device='cuda') if want_Y else None
    rec, = KN.dopri5_fwd([dict(xT=xT, start=s, u=u, Y=Y)], t, blob, Hc, Kc, m, H, stepper=stepper, **kw)
    return dict(u=u, Y=Y, rec=rec, xT=xT, t=t, s=s, blob=blob, Hc=Hc, Kc=Kc)


# (d, H, K, m, N, L, seed, factor on the start values): tanh-only fields, the step decisions pinned exactly.  Attempts / accepted /
# gap = min |ratio - 1| of the restatement on the CPU: 8/8 4.3e-1, 8/8 4.0e-1, 8/8 4.2e-1, 9/9 3.9e-1, 7/7 4.7e-2, 8/8 4.6e-1,
# 7/7 2.0e-1, 7/7 3.7e-1 (container width), 7/7 4.3e-1 (wide container), 8/7 1.9e-1 (one REJECTED attempt) -- the smallest gap is
# seven orders above what rounding moves the ratio by
WIDE_SMOOTH = [(5, 128, 32, 1, 37, 5, 101, 1.0), (20, 128, 64, 1, 37, 6, 102, 1.0), (3, 96, 32, 1, 50, 4, 103, 1.0),
               (20, 256, 256, 1, 19, 4, 104, 1.0), (4, 65, 16, 1, 1, 5, 105, 1.0), (20, 128, 64, 1, 1000, 5, 106, 1.0),
               (20, 20, 17, 1, 4096, 6, 107, 1.0), (3, 20, 10, 1, 37, 5, 108, 1.0), (20, 64, 16, 1, 100, 6, 109, 1.0),
               (5, 128, 32, 1, 37, 5, 101, 100.0)]
WIDE_COUNTS = [(8, 8), (8, 8), (8, 8), (9, 9), (7, 7), (8, 8), (7, 7), (7, 7), (7, 7), (8, 7)]


def _check_forward(d, H, K, m, N, L, seed, factor=1.0):
    cfg, theta, X, start = _case(d, H, K, m, N, L, seed)
    start = start * factor
    ys, info = _ref_Y(theta, cfg, X, start)
    assert info['gap'] > 1e-9, 'bad fixture: a step decision within %.1e of the threshold' % info['gap']
    u_ref = (ys @ theta['FL_w'].T + theta['FL_b']).squeeze(2)
    g = _gpu_fwd(theta, X, start, d, H, K, m)
    rec = g['rec']
    print('forward', (d, H, K, m, N, L, seed, factor), 'device', (rec.n_att, rec.n_acc), 'ref', (info['n_att'], info['n_acc']),
          'gap', info['gap'], 'grid', _rel(rec.grid, _grid_of(info)) if rec.n_acc == info['n_acc'] else None,
          'u', _rel(g['u'].t(), u_ref), 'Y', _rel(g['Y'][:, :H, :].permute(2, 0, 1), ys))
    assert (rec.n_att, rec.n_acc) == (info['n_att'], info['n_acc'])
    assert _rel(rec.grid, _grid_of(info)) < GRID_TOL
    assert _rel(g['u'].t(), u_ref) < 1e-9
    assert _rel(g['Y'][:, :H, :].permute(2, 0, 1), ys) < 1e-9
    if g['Hc'] > H:
        assert float(g['Y'][:, H:, :].abs().max()) == 0.0                 # the padding units stay exactly zero
    return info


@pytest.mark.parametrize('case,counts', list(zip(WIDE_SMOOTH, WIDE_COUNTS)))
def test_forward_against_the_restatement(case, counts):
    info = _check_forward(*case)
    assert (info['n_att'], info['n_acc']) == counts                       # (the fixture is the one that was checked)


@pytest.mark.parametrize('d,H,K,m,N,L,seed', SMOOTH_CASES)
def test_forward_against_the_restatement_at_container_widths(d, H, K, m, N, L, seed):
    _check_forward(d, H, K, m, N, L, seed)


# ReLU fields: the step sequence is not a smooth function of the rounding (tests/test_gpu_dopri5.py), so the arithmetic is pinned on
# the device's own accepted grid.  The restatement alone, on the CPU: 22/21, 23/23, 16/16, 43/42, 15/13, 49/31 attempts / accepted.
WIDE_RELU = [(5, 128, 32, 8, 37, 5, 111), (20, 128, 64, 8, 37, 6, 112), (3, 96, 32, 12, 20, 4, 113), (6, 256, 128, 4, 19, 3, 114),
             (20, 48, 16, 11, 33, 5, 115), (4, 20, 10, 8, 37, 5, 116)]


@pytest.mark.parametrize('d,H,K,m,N,L,seed', WIDE_RELU)
def test_forward_relu_field_on_its_own_grid(d, H, K, m, N, L, seed):
    cfg, theta, X, start = _case(d, H, K, m, N, L, seed)
    g = _gpu_fwd(theta, X, start, d, H, K, m)
    rec = g['rec']
    ys, _ = _ref_Y(theta, cfg, X, start, frozen=rec.steps)
    ys2, info = _ref_Y(theta, cfg, X, start)
    got = g['Y'][:, :H, :].permute(2, 0, 1)
    print('relu', (d, H, K, m, N, L, seed), 'device', (rec.n_att, rec.n_acc), 'ref', (info['n_att'], info['n_acc']),
          'u', _rel(g['u'].t(), (ys @ theta['FL_w'].T + theta['FL_b']).squeeze(2)), 'Y', _rel(got, ys), 'free', _rel(got, ys2))
    assert _rel(g['u'].t(), (ys @ theta['FL_w'].T + theta['FL_b']).squeeze(2)) < 1e-9
    assert _rel(got, ys) < 1e-9
    # ... and both solves are within tolerance of each other
    assert _rel(got, ys2) < 1e-4
    assert abs(rec.n_acc - info['n_acc']) <= max(3, info['n_acc'] // 5) and rec.n_att >= rec.n_acc


def _sweep(g, job, d, m, stepper, want_x=True, want_params=True, ones=False):
    from xnode_wan_pde_solver_amd import kernels as KN
    N = g['xT'].shape[1]
    P = KN.theta_size(d, g['Hc'], g['Kc'])
    job = dict(job)
    if want_x:
        job.update(gx=torch.full((d, N), float('nan'), dtype=F64, device='cuda'), gs=torch.full((N,), float('nan'), dtype=F64, device='cuda'))
    if want_params:
        job['gslab'] = torch.full((KN.ode_bwd_slabs(N), P), float('nan'), dtype=F64, device='cuda')
    KN.dopri5_sweep([job], g['t'], g['blob'], g['Hc'], g['Kc'], m, want_x=want_x, want_params=want_params, x_cot_ones=ones,
                    stepper=stepper)
    return job


@pytest.mark.parametrize('d,H,K,m,N,L,seed', SMOOTH_CASES)
def test_against_the_vector_implementation(d, H, K, m, N, L, seed):
    """the widths both serve: same counts, grids and u; and the sweeps crossed -- each sweep on the other forward's record"""
    from xnode_wan_pde_solver_amd import kernels as KN
    cfg, theta, X, start = _case(d, H, K, m, N, L, seed)
    gt = _gpu_fwd(theta, X, start, d, H, K, m, stepper='tiled')
    gv = _gpu_fwd(theta, X, start, d, H, K, m, stepper='vector')
    assert (gt['rec'].n_att, gt['rec'].n_acc) == (gv['rec'].n_att, gv['rec'].n_acc)
    assert _rel(gt['rec'].grid, gv['rec'].grid) < GRID_TOL
    assert _rel(gt['u'], gv['u']) < 1e-9 and _rel(gt['Y'], gv['Y']) < 1e-9
    ubar = torch.randn(L, N, dtype=F64, generator=torch.Generator().manual_seed(seed + 7)).cuda()
    for g, own, other in ((gv, 'vector', 'tiled'), (gt, 'tiled', 'vector')):
        job = dict(xT=g['xT'], start=g['s'], rec=g['rec'], ubar=ubar)
        a = _sweep(g, job, d, m, own)
        b = _sweep(g, job, d, m, other)
        fa, fb = KN.slab_sum(a['gslab']), KN.slab_sum(b['gslab'])
        print('crossed', (d, H, K, m, N, L, seed), own, 'record swept by', other, _rel(fb, fa), _rel(b['gx'], a['gx']), _rel(b['gs'], a['gs']))
        assert float(fa.abs().max()) > 0 and _rel(fb, fa) < 1e-9
        assert _rel(b['gx'], a['gx']) < 1e-9 and _rel(b['gs'], a['gs']) < 1e-9


SWEEP_CASES = [(4, 128, 32, 8, 37, 5, 131), (3, 96, 32, 2, 20, 4, 132), (6, 256, 64, 12, 19, 3, 133), (4, 20, 10, 8, 37, 5, 31)]


@pytest.mark.parametrize('d,H,K,m,N,L,seed', SWEEP_CASES)
@pytest.mark.parametrize('form', ['ubar', 'ones_x', 'res', 'res_first', 'weak'])
def test_sweep_against_frozen_grid_autograd(d, H, K, m, N, L, seed, form):
    from xnode_wan_pde_solver_amd import kernels as KN, nets
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
    ones = form == 'ones_x'
    full = _sweep(g, job, d, m, 'tiled', ones=ones)
    flat = KN.slab_sum(full['gslab']).cpu()
    # the parameter gradients, at the network's own widths
    slots, _ = nets._u_slots(d, H, K, g['Hc'], g['Kc'], m > 1)
    keys = [k for k in U_ORDER if m > 1 or k not in ('Wh', 'Wh_b')]
    worst = 0.0
    for k, (off, r, c, ld) in zip(keys, slots):
        got = torch.stack([flat[off + i * ld:off + i * ld + c] for i in range(r)]).reshape(gp_r[k].shape)
        worst = max(worst, _rel(got, gp_r[k]))
        assert float(gp_r[k].abs().max()) > 0, k                           # (not a comparison of zeros)
        assert _rel(got, gp_r[k]) < 1e-9, (form, k, _rel(got, gp_r[k]))
    if ones:                                                                # x-side outputs of the all-ones cotangent
        _, gx_r, gs_r, _ = _ref_grads(theta, cfg, X, start, lambda u: u.sum(), g['rec'].steps)
    print('sweep', (d, H, K, m, N, L, seed), form, 'steps', (g['rec'].n_att, g['rec'].n_acc), 'params', worst,
          'gx', _rel(full['gx'].t(), gx_r), 'gs', _rel(full['gs'], gs_r))
    assert _rel(full['gx'].t(), gx_r) < 1e-9, form
    assert _rel(full['gs'], gs_r) < 1e-9, form
    # x-only and params-only calls: the same bits as the combined call for the outputs they share
    po = _sweep(g, job, d, m, 'tiled', want_x=False)
    assert torch.equal(po['gslab'], full['gslab'])
    if not ones:                                                            # (x_cot_ones needs both outputs)
        xo = _sweep(g, job, d, m, 'tiled', want_params=False)
        assert torch.equal(xo['gx'], full['gx']) and torch.equal(xo['gs'], full['gs'])


def _two_jobs(d, H, K, m, L):
    cfg, theta, X1, s1 = _case(d, H, K, m, 40, L, 21)
    _, _, X2, s2 = _case(d, H, K, m, 70, L, 22)
    X2 = X2.clone()
    X2[:, :, 0] = X1[0, :, 0].view(1, L)                                    # (the jobs of a launch share t)
    return cfg, theta, (X1, s1), (X2, 100.0 * s2)                           # a larger start: more attempts


@pytest.mark.parametrize('d,H,K,m,L', [(5, 20, 10, 1, 6), (5, 128, 32, 1, 6)])
def test_two_jobs_with_their_own_controllers(d, H, K, m, L):
    """two jobs in one launch that need different numbers of steps: each equals the same job run alone (to the bit) and the
    restatement (tanh field: the step decisions too)"""
    from xnode_wan_pde_solver_amd import kernels as KN
    cfg, theta, a, b = _two_jobs(d, H, K, m, L)
    blob, Hc, Kc = _blob(theta, d, H, K, m)
    t = a[0][0, :, 0].double().cuda()
    jobs = [dict(xT=X[:, 0, 1:].double().t().contiguous().cuda(), start=s.cuda(), u=torch.empty(L, X.shape[0], dtype=F64, device='cuda'))
            for X, s in (a, b)]
    recs = KN.dopri5_fwd(jobs, t, blob, Hc, Kc, m, H, stepper='tiled')
    assert (recs[0].n_att, recs[0].n_acc) != (recs[1].n_att, recs[1].n_acc)
    for rec, (X, s), j in zip(recs, (a, b), jobs):
        ys, info = _ref_Y(theta, cfg, X, s)
        assert info['gap'] > 1e-9
        assert (rec.n_att, rec.n_acc) == (info['n_att'], info['n_acc'])
        assert _rel(rec.grid, _grid_of(info)) < GRID_TOL
        assert _rel(j['u'].t(), (ys @ theta['FL_w'].T + theta['FL_b']).squeeze(2)) < 1e-9
        alone = _gpu_fwd(theta, X, s, d, H, K, m, want_Y=False)
        assert torch.equal(alone['u'], j['u']) and torch.equal(alone['rec'].grid, rec.grid)
    # the sweep of both jobs in one launch: each job's outputs are those of its own launch, to the bit
    ubars = [torch.randn(L, j['xT'].shape[1], dtype=F64, generator=torch.Generator().manual_seed(5 + i)).cuda() for i, j in enumerate(jobs)]
    P = KN.theta_size(d, Hc, Kc)
    sj = [dict(xT=j['xT'], start=j['start'], rec=r, ubar=ub, gx=torch.empty(d, j['xT'].shape[1], dtype=F64, device='cuda'),
               gs=torch.empty(j['xT'].shape[1], dtype=F64, device='cuda'),
               gslab=torch.empty(KN.ode_bwd_slabs(j['xT'].shape[1]), P, dtype=F64, device='cuda')) for j, r, ub in zip(jobs, recs, ubars)]
    KN.dopri5_sweep(sj, t, blob, Hc, Kc, m, want_x=True, want_params=True, stepper='tiled')
    for j in sj:
        one = dict(j, gx=torch.empty_like(j['gx']), gs=torch.empty_like(j['gs']), gslab=torch.empty_like(j['gslab']))
        KN.dopri5_sweep([one], t, blob, Hc, Kc, m, want_x=True, want_params=True, stepper='tiled')
        assert torch.equal(one['gx'], j['gx']) and torch.equal(one['gs'], j['gs']) and torch.equal(one['gslab'], j['gslab'])


def test_eight_jobs_in_one_launch_and_nine_raise():
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    d, H, K, m, L = 4, 65, 16, 1, 4
    cfg, theta, X0, _ = _case(d, H, K, m, 8, L, 71)
    blob, Hc, Kc = _blob(theta, d, H, K, m)
    t = X0[0, :, 0].double().cuda()
    samples = []
    for i in range(9):
        N = (1, 16, 17, 37, 5, 64, 33, 100, 8)[i]
        _, _, X, s = _case(d, H, K, m, N, L, 72 + i)
        X = X.clone()
        X[:, :, 0] = X0[0, :, 0].view(1, L)
        samples.append((X, s * (1.0 + 3.0 * i)))
    jobs = [dict(xT=X[:, 0, 1:].double().t().contiguous().cuda(), start=s.cuda(), u=torch.empty(L, X.shape[0], dtype=F64, device='cuda'))
            for X, s in samples]
    recs = KN.dopri5_fwd(jobs[:8], t, blob, Hc, Kc, m, H, stepper='tiled')
    for rec, (X, s), j in zip(recs, samples, jobs):
        alone = _gpu_fwd(theta, X, s, d, H, K, m, want_Y=False)
        assert (alone['rec'].n_att, alone['rec'].n_acc) == (rec.n_att, rec.n_acc)
        assert torch.equal(alone['u'], j['u']) and torch.equal(alone['rec'].grid, rec.grid)
    with pytest.raises(XnwanError, match='1 .. 8 jobs'):
        KN.dopri5_fwd(jobs, t, blob, Hc, Kc, m, H, stepper='tiled')
    with pytest.raises(XnwanError, match='1 .. 8 jobs'):
        KN.dopri5_sweep([dict(j, rec=recs[0]) for j in jobs], t, blob, Hc, Kc, m, True, False, stepper='tiled')


def test_record_growth_gives_the_same_results():
    d, H, K, m, N, L = 4, 96, 32, 8, 50, 5
    cfg, theta, X, start = _case(d, H, K, m, N, L, 41)
    a = _gpu_fwd(theta, X, start, d, H, K, m, rtol=1e-10, atol=1e-12, cap=2, chunk=3)
    b = _gpu_fwd(theta, X, start, d, H, K, m, rtol=1e-10, atol=1e-12, cap=4000)
    assert a['rec'].n_acc > 20 and a['rec'].cap > 2
    assert torch.equal(a['u'], b['u']) and torch.equal(a['Y'], b['Y']) and torch.equal(a['rec'].grid, b['rec'].grid)
    assert a['rec'].n_att == b['rec'].n_att


def test_step_limit_raises():
    from xnode_wan_pde_solver_amd._lib import XnwanError
    d, H, K, m, N, L = 4, 96, 32, 8, 16, 4
    cfg, theta, X, start = _case(d, H, K, m, N, L, 51)
    with pytest.raises(XnwanError, match='step limit of 3 accepted steps'):
        _gpu_fwd(theta, X, start, d, H, K, m, max_steps=3)


def test_a_forward_run_twice_gives_the_same_bits():
    d, H, K, m, N, L = 5, 128, 32, 8, 1000, 5
    cfg, theta, X, start = _case(d, H, K, m, N, L, 52)
    a = _gpu_fwd(theta, X, start, d, H, K, m)
    b = _gpu_fwd(theta, X, start, d, H, K, m)
    assert a['rec'].n_acc >= 1 and (a['rec'].n_att, a['rec'].n_acc) == (b['rec'].n_att, b['rec'].n_acc)
    assert torch.equal(a['u'], b['u']) and torch.equal(a['Y'], b['Y']) and torch.equal(a['rec'].grid, b['rec'].grid)
    n = a['rec'].n_acc
    assert torch.equal(a['rec'].rec_y[:n + 1], b['rec'].rec_y[:n + 1]) and torch.equal(a['rec'].rec_h[:n], b['rec'].rec_h[:n])
    assert not bool(torch.isnan(a['u']).any()) and not bool(torch.isnan(a['Y']).any())


def test_autograd_surface_and_determinism():
    """u_net(X).sum().backward() with solver 'dopri5' on the tiled stepper at (128, 32, 8) against the restatement's frozen-grid
    autograd; twice, bit-identical"""
    from xnode_wan_pde_solver_amd import nets
    d, H, K, m, N, L = 4, 128, 32, 8, 96, 8
    cfg, theta, X, start = _case(d, H, K, m, N, L, 61)
    setup = {'dim': d, 'T0': 0, 'T': 1}
    h = lambda Z: start.view(-1, 1).to(Z.device)                            # noqa: E731  (the start values of this sample)
    net = nets.XNODE(H, 1, h, None, setup, K, m, None, solver='dopri5')
    net.dopri5_stepper = 'tiled'
    named = dict(net.named_parameters())
    from oracle import refspec as R
    with torch.no_grad():
        for name, key in R.u_names(m):
            named[name[len('module.'):]].copy_(theta[key].reshape(named[name[len('module.'):]].shape))
    net.bind(torch.device('cuda'))
    assert net.family == 'tiled' and net.kdims == (H, K)
    runs = []
    for _ in range(2):
        net.zero_grad()
        Xc = X.cuda().requires_grad_(True)
        u = net(Xc, starts_at_T0=True)
        u.sum().backward()
        runs.append((u.detach().clone(), Xc.grad.clone(), [p.grad.clone() for p in net.parameters()]))
    assert net.last_dopri5.stepper == 'tiled'
    u_r, gx_r, _, gp_r = _ref_grads(theta, cfg, X, start, lambda u: u.sum(), net.last_dopri5.steps)
    assert _rel(runs[0][0].squeeze(2), u_r) < 1e-9
    assert _rel(runs[0][1][:, 0, 1:], gx_r) < 1e-6                         # (X is float32, the reference's cube sample: so is its gradient)
    for (name, key), p in zip(R.u_names(m), net.parameters()):
        assert _rel(p.grad, gp_r[key].reshape(p.shape)) < 1e-9, name
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
