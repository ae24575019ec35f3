"""Rates of solver 'explicit_adams' on the tiled stepper family (csrc/xw_tiled.hip) against tiled midpoint and rk4: kernel times
of the forward pass and the sweep (with weight gradients) at the headline sample (d = 20, 2 x 4096 paths, N_t = 32), field
evaluations per step, and engine sub-steps per second.  python tools/adams_rate.py [--quick]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xnode_wan_pde_solver_amd import kernels as KN          # noqa: E402

F64 = torch.float64
NAMES = {1: 'midpoint', 2: 'rk4', KN.ADAMS: 'explicit_adams'}


def field_evals(method, L):
    """field evaluations of one forward pass over L grid points (explicit_adams: 4 in each rk4 start-up step, then 1)"""
    if method == KN.ADAMS:
        return sum(4 if n < 2 else 1 for n in range(L - 1))
    return {0: 1, 1: 2, 2: 4}[method] * (L - 1)


def kernel_times(d, H, K, m, method, L, N, reps):
    dev = torch.device('cuda')
    P = KN.theta_size(d, H, K)
    g = torch.Generator().manual_seed(0)
    theta = (0.1 * torch.randn(P, generator=g, dtype=F64)).to(dev)
    xT = (torch.rand(d, N, generator=g, dtype=F64) * 2 - 1).to(dev)
    t = torch.linspace(0, 1, L, dtype=F64, device=dev)
    start = torch.randn(N, dtype=F64, generator=g).to(dev)
    job = dict(xT=xT, start=start, u=torch.empty(L, N, dtype=F64, device=dev), Y=torch.empty(L, H, N, dtype=F64, device=dev))
    gx, gs = torch.empty(d, N, dtype=F64, device=dev), torch.empty(N, dtype=F64, device=dev)
    slab = torch.empty(KN.ode_bwd_slabs(N), P, dtype=F64, device=dev)
    ubar = torch.ones(L, N, dtype=F64, device=dev)
    fwd = lambda: KN.tiled_ode_fwd_multi([job], t, theta, method, H, K, m)                           # noqa: E731
    bwd = lambda: KN.tiled_ode_bwd_multi([dict(job, ubar=ubar, gx=gx, gs=gs, gslab=slab)], t, theta, method, H, K, m,  # noqa: E731
                                         want_x=True, want_params=True)
    out = {}
    for name, fn in (('fwd', fwd), ('bwd', bwd)):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name] = e0.elapsed_time(e1) / reps
    ev = field_evals(method, L)
    print('%-14s (H, K, m) = (%d, %d, %d) d %d L %d N %d: forward %.3f ms, sweep %.3f ms, together %.3f ms; %d field evaluations '
          'per path, %.2f us of forward per evaluation' % (NAMES[method], H, K, m, d, L, N, out['fwd'], out['bwd'],
                                                            out['fwd'] + out['bwd'], ev, out['fwd'] / ev * 1e3), flush=True)
    return out


def substep_rate(Hh, Kk, m, solver, d=20, N=4096, L=32, steps=10):
    import configs.Ex4_1_funcs as P
    from src.training import NODE_WAN_solver
    from src.dataset import Comb_loader
    params = {'alpha': 1e8, 'u_layers': m, 'u_hidden_dim': Hh, 'u_hidden_hidden_dim': Kk, 'v_layers': 9, 'v_hidden_dim': 50,
              'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': solver,
              'dim': d, 'N_t': L, 'N_r': N, 'N_b': N, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 1, 'domain': 'Hypercube'}
    torch.manual_seed(0)
    S = NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, torch.device('cuda'), './',
                        func_u_sol=P.func_u_sol, p=2)
    s = S.setup
    domain = S.domain(s['shape_param'], s['dim'], s['T0'], s['T'], s['N_t'])
    pts = Comb_loader(s['N_r'], s['N_b'], domain, S.device)
    G = S.engine.load_group(pts.interioru, pts.interiorv, pts.boundary, domain)
    for _ in range(2):
        S.engine.generator_step(G)
        S.engine.discriminator_step(G)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        S.engine.generator_step(G)
        S.engine.discriminator_step(G)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print('sub-steps (%d, %d, %d) %-14s d %d N %d L %d stepper %s: %.2f sub-steps/s (%.3f ms each)'
          % (Hh, Kk, m, solver, d, N, L, S.engine.stepper, 2 * steps / dt, dt / (2 * steps) * 1e3), flush=True)


if __name__ == '__main__':
    quick = '--quick' in sys.argv
    reps = 3 if quick else 10
    for H, K, m in ((20, 10, 8), (128, 64, 8)):
        for method in (1, 2, KN.ADAMS):
            kernel_times(20, H, K, m, method, 32, 8192, reps)
    for H, K, m in ((20, 10, 8), (128, 64, 8)):
        for solver in ('midpoint', 'rk4', 'explicit_adams'):
            substep_rate(H, K, m, solver, steps=3 if quick else 10)
