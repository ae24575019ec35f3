"""Rates of the tiled stepper family (csrc/xw_tiled.hip): kernel times of its forward pass and sweep, their fraction of the
FP64 matrix peak, and engine sub-steps per second at widths only it serves -- plus the tiled family against the generic path
at (64, 16, 12).  python tools/tiled_rate.py [--quick]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xnode_wan_pde_solver_amd import kernels as KN          # noqa: E402
from xnode_wan_pde_solver_amd.options import EngineOptions  # noqa: E402

PEAK = 78.6e12
F64 = torch.float64


def field_flops(d, H, K, m, method, L, N):
    """2 x multiply-adds of the field layers (x-projection hoisted) x stages x steps x paths"""
    stages = {0: 1, 1: 2, 2: 4}[method]
    return 2.0 * (K * (H + 1) + (m - 1) * K * K + H * K) * stages * (L - 1) * N


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
    out = {}
    for fam in ('tiled', 'generic') if KN.stepper_family(H, K, m) == 'generic' else ('tiled',):
        fwd = (lambda: KN.tiled_ode_fwd_multi([job], t, theta, method, H, K, m)) if fam == 'tiled' else \
              (lambda: KN.ode_fwd_multi([job], t, theta, method, H, K, m))
        bw = KN.tiled_ode_bwd_multi if fam == 'tiled' else KN.ode_bwd_multi
        bwd = lambda: bw([dict(job, ubar=ubar, gx=gx, gs=gs, gslab=slab)], t, theta, method, H, K, m, want_x=True, want_params=True)  # noqa: E731
        for name, fn in (('fwd', fwd), ('bwd', bwd)):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / reps
            fl = field_flops(d, H, K, m, method, L, N)
            out[(fam, name)] = ms
            print('%-7s %s (H, K, m) = (%d, %d, %d) d %d L %d N %d method %d: %.3f ms, %.2f TFLOP/s = %.3f of FP64 peak'
                  % (fam, name, H, K, m, d, L, N, method, ms, fl / ms * 1e-9, fl / ms * 1e-9 / (PEAK * 1e-12)), flush=True)
    return out


def substep_rate(Hh, Kk, m, d, N, L, steps, options=None):
    import configs.Ex4_1_funcs as P
    from src.training import NODE_WAN_solver
    from src.dataset import Comb_loader
    params = {'alpha': 1e8, 'u_layers': m, 'u_hidden_dim': Hh, 'u_hidden_hidden_dim': Kk, 'v_layers': 9, 'v_hidden_dim': 50,
              'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'midpoint',
              'dim': d, 'N_t': L, 'N_r': N, 'N_b': N, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 1, 'domain': 'Hypercube'}
    torch.manual_seed(0)
    S = NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, torch.device('cuda'), './',
                        func_u_sol=P.func_u_sol, p=2, options=options)
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
    print('sub-steps (%d, %d, %d) d %d N %d L %d stepper %s: %.2f sub-steps/s (%.3f ms each)'
          % (Hh, Kk, m, d, N, L, S.engine.stepper, 2 * steps / dt, dt / (2 * steps) * 1e3), flush=True)


if __name__ == '__main__':
    quick = '--quick' in sys.argv
    reps = 3 if quick else 10
    for H, K, m in ((64, 32, 8), (128, 64, 8), (256, 128, 4), (64, 16, 12)):
        kernel_times(20, H, K, m, 1, 32, 4096, reps)
    for H, K, m in ((64, 32, 8), (128, 64, 8), (256, 128, 4)):
        substep_rate(H, K, m, 20, 4096, 32, 3 if quick else 10)
    substep_rate(64, 16, 12, 20, 4096, 32, 1 if quick else 3)
    substep_rate(64, 16, 12, 20, 4096, 32, 3 if quick else 10, EngineOptions(tiled_stepper='generic'))
