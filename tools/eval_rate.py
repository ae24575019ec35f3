"""Cost of evaluating u at scattered points (NODE_WAN_solver.evaluate, csrc/xw_tiled_paths.hip) against what there was before:
the README recipe u_net([[x0, x]]) point by point, and one shared-time call through domain.bound_pad.  Workload: the YAML network
(20, 10, 8), midpoint, N_t = 20, d = 20, M uniform random points of the cube x [T0, T].
python tools/eval_rate.py [--points M] [--reps R]        (one JSON line at the end)"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import configs.Ex4_1_funcs as P                                    # noqa: E402
from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN   # noqa: E402

F64 = torch.float64


def timed(fn, reps):
    """median wall time of fn() in ms, each call ended by a device synchronise; one warm-up"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def padded_work(n):
    """sum over 16-path tiles of 16 max(n) over sum n, for the points in the given order"""
    pad = (-n.numel()) % 16
    tiles = torch.cat((n, n.new_zeros(pad))).view(-1, 16)
    return float(16 * tiles.max(1).values.sum()) / max(float(n.sum()), 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=131072)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    from src.training import NODE_WAN_solver
    d, M = 20, a.points
    params = {'alpha': 1e8, 'u_layers': 8, 'u_hidden_dim': 20, 'u_hidden_hidden_dim': 10, 'v_layers': 9, 'v_hidden_dim': 50,
              'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'midpoint',
              'dim': d, 'N_t': 20, 'N_r': 4000, 'N_b': 4000, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 1,
              'domain': 'Hypercube'}
    torch.manual_seed(0)
    S = NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, torch.device('cuda'), './',
                        func_u_sol=P.func_u_sol, p=2)
    dev = S.device
    g = torch.Generator().manual_seed(1)
    pts = torch.cat((torch.rand(M, 1, generator=g, dtype=F64), torch.rand(M, d, generator=g, dtype=F64) * 2 - 1), 1)
    pts_dev = pts.to(dev)
    out = {'points': M, 'family_trained': S.engine.stepper}

    # 1. evaluate: host points (upload included) and device points
    out['evaluate_ms_host_points'] = timed(lambda: S.evaluate(pts), a.reps)
    out['evaluate_ms_device_points'] = timed(lambda: S.evaluate(pts_dev), a.reps)

    # 2. padded work with and without the sort
    n = EP.step_counts(pts[:, 0], torch.zeros(M, dtype=F64), 0, 1, params['N_t'])
    order, _ = EP.sort_by_steps(n)
    out['steps_total'] = int(n.sum())
    out['padded_work_unsorted'] = padded_work(n)
    out['padded_work_sorted'] = padded_work(n[order])

    # ... and the launch chain without the sort (the kernel on the unsorted points, nstep hint kept)
    tT = EP.pack_grids(pts_dev[:, 0].contiguous(), torch.zeros(M, dtype=F64, device=dev), n.to(dev))
    xT = pts_dev[:, 1:].t().contiguous()
    s = P.func_h(torch.cat((torch.zeros(M, 1, dtype=F64, device=dev), pts_dev[:, 1:]), 1)).contiguous()
    th, (H, K), m = S.engine.theta.data, S.u_net.module.kdims, 8
    n32 = n.to(torch.int32).to(dev)
    out['kernel_ms_unsorted'] = timed(lambda: EP.paths_forward(xT, tT, s, n32, th, 1, H, K, m, last_only=True), a.reps)
    o = order.to(dev)
    xs, ts_, ss, ns = xT[:, o].contiguous(), tT[:, o].contiguous(), s[o].contiguous(), n32[o].contiguous()
    out['kernel_ms_sorted'] = timed(lambda: EP.paths_forward(xs, ts_, ss, ns, th, 1, H, K, m, last_only=True), a.reps)

    # 3. before: the README recipe, one point per call, over 256 of the points
    def recipe():
        with torch.no_grad():
            for i in range(256):
                x0 = pts[i].clone()
                x0[0] = 0.0
                S.u_net(torch.stack((x0, pts[i])).unsqueeze(0))
    out['recipe_ms_per_point'] = timed(recipe, max(1, a.reps // 2)) / 256

    # 4. before: ONE shared time for all M points through bound_pad (the fused container) -- and evaluate on the same slice
    slab = pts.clone()
    slab[:, 0] = 0.62
    X1 = slab.unsqueeze(1)

    def shared():
        with torch.no_grad():
            S.u_net(X1)
    out['bound_pad_one_time_ms'] = timed(shared, a.reps)
    out['evaluate_one_time_ms'] = timed(lambda: S.evaluate(slab), a.reps)

    # 5. the kernel against kt_ode_fwd on a shared grid: per field evaluation (midpoint: two per step)
    L, Nk = 21, min(M, 65536)
    t = torch.linspace(0, 1, L, dtype=F64, device=dev)
    xk, sk = xT[:, :Nk].contiguous(), s[:Nk].contiguous()
    tk = t.view(L, 1).expand(L, Nk).contiguous()
    u = torch.empty(L, Nk, dtype=F64, device=dev)
    ms_pp = timed(lambda: KN.tiled_paths_fwd([dict(xT=xk, start=sk, tT=tk, u=u)], th, 1, H, K, m), a.reps)
    ms_one = timed(lambda: KN.tiled_ode_fwd_multi([dict(xT=xk, start=sk, u=u)], t, th, 1, H, K, m), a.reps)
    evals = Nk * (L - 1) * 2
    out['kt_ode_fwd_pp_ns_per_field_eval'] = ms_pp * 1e6 / evals
    out['kt_ode_fwd_ns_per_field_eval'] = ms_one * 1e6 / evals
    out['shared_grid_paths'] = Nk
    print(json.dumps(out))


if __name__ == '__main__':
    main()
