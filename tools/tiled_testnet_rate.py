"""Rates of the tiled test-network family (csrc/xw_disc_tiled.hip): kernel times of its forward pass (with the record and the
fused input gradient at the first time index, as in the engine's sub-steps) and its reverse, their fraction of the FP64 matrix
peak, the tiled family against the MFMA container at W = 128, and engine sub-steps per second next to two stepper families.
Headline sample: d = 20, 4096 paths x 32 times.
    python tools/tiled_testnet_rate.py [--quick] [--kernels-only] [--w256 (one kernel shape, for a counter pass)]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xnode_wan_pde_solver_amd import kernels as KN          # noqa: E402

PEAK = 78.6e12
F64 = torch.float64


def macs(d, W, q):
    return (d + 1) * W + q * W * W + W


def kernel_times(d, W, q, L, N, reps, family):
    """profiles/r06_disc_widths.txt: forward 2 (2 P + N) MACs, reverse 4 P MACs (P = N L points)"""
    dev = torch.device('cuda')
    g = torch.Generator().manual_seed(0)
    phi = (0.1 * torch.randn(KN.phi_size(d, W), generator=g, dtype=F64)).to(dev)
    xT = (torch.rand(d, N, generator=g, dtype=F64) * 2 - 1).to(dev)
    t = torch.linspace(0, 1, L, dtype=F64, device=dev)
    v = torch.empty(L, N, dtype=F64, device=dev)
    vt = torch.empty_like(v)
    gxv, gtv = torch.empty(d, N, dtype=F64, device=dev), torch.empty(N, dtype=F64, device=dev)
    act = torch.empty(KN.disc_act_rows(W, q, family), KN.disc_act_cols(L * N), dtype=F64, device=dev)
    slab = torch.empty(KN.disc_bwd_slabs(N, L), phi.numel(), dtype=F64, device=dev)
    vbar = torch.ones(L, N, dtype=F64, device=dev)
    xp = KN.disc_xproj(xT, phi, W) if family == 'mfma' else None
    fwd = lambda: KN.disc_fwd(xT, t, phi, W, q, v=v, vt=vt, gxv=gxv, gtv=gtv, ngrad=N, act=act, xproj=xp, family=family)  # noqa: E731
    bwd = lambda: KN.disc_bwd(xT, t, phi, vbar, W, q, gslab=slab, act=act, family=family)                              # noqa: E731
    P = L * N
    out = {}
    for name, fn, fl in (('fwd+record', fwd, 2.0 * (2 * P + N) * macs(d, W, q)), ('reverse', bwd, 4.0 * P * macs(d, W, q))):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        out[name] = ms
        print('%-5s %-10s W %d q %d d %d L %d N %d: %.3f ms, %.2f TFLOP/s = %.3f of FP64 peak'
              % (family, name, W, q, d, L, N, ms, fl / ms * 1e-9, fl / ms * 1e-9 / (PEAK * 1e-12)), flush=True)
    return out


def substep_rate(Hh, Kk, m, W, q, d, N, L, steps):
    import configs.Ex4_1_funcs as P
    from src.training import NODE_WAN_solver
    from src.dataset import Comb_loader
    params = {'alpha': 1e8, 'u_layers': m, 'u_hidden_dim': Hh, 'u_hidden_hidden_dim': Kk, 'v_layers': q, 'v_hidden_dim': W,
              'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'midpoint',
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
    print('sub-steps u (%d, %d, %d) + v (%d, %d) d %d N %d L %d stepper %s testnet %s: %.2f sub-steps/s (%.3f ms each)'
          % (Hh, Kk, m, W, q, d, N, L, S.engine.stepper, S.engine.testnet, 2 * steps / dt, dt / (2 * steps) * 1e3), flush=True)


if __name__ == '__main__':
    quick = '--quick' in sys.argv or '--kernels-only' in sys.argv
    reps = 2 if quick else 5
    if '--w256' in sys.argv:                          # (one shape: a counter pass)
        kernel_times(20, 256, 9, 32, 4096, 1, 'tiled')
        sys.exit(0)
    for W, q in ((256, 9), (256, 20), (192, 9), (192, 20)):
        kernel_times(20, W, q, 32, 4096, reps, 'tiled')
    for fam in ('mfma', 'tiled'):
        kernel_times(20, 128, 9, 32, 4096, reps, fam)
    if '--kernels-only' in sys.argv:
        sys.exit(0)
    substep_rate(20, 10, 8, 256, 9, 20, 4096, 32, 2 if quick else 5)
    substep_rate(128, 64, 8, 256, 9, 20, 4096, 32, 2 if quick else 5)
