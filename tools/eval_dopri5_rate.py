"""Cost of evaluate() with solver 'dopri5' (a step controller per path, csrc/xw_tdopri_paths.hip) against what a user had before,
in one process: the README recipe with dopri5 -- one XNODE.forward per point, on a sample of the points -- and midpoint evaluate at
N_t.  Workload: the YAML network (20, 10, 8) at its initial weights, d = 20, M uniform random points of the cube x [T0, T].
python tools/eval_dopri5_rate.py [--points M] [--reps R] [--recipe-points Q]        (one JSON line at the end)"""
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
SPREAD = {}                                                        # name -> [min, max] ms of the repetitions behind a median


def timed(fn, reps, name=None):
    """median wall time of fn() in ms, each call ended by a device synchronise; one warm-up"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    if name:
        SPREAD[name] = [round(min(ts), 3), round(max(ts), 3)]
    return sorted(ts)[len(ts) // 2]


def tile_rounds(n_att):
    """rounds per 16-path tile (the tile walks until its last path is done): int64 [tiles], for the points in the given order"""
    pad = (-n_att.numel()) % 16
    return torch.cat((n_att, n_att.new_zeros(pad))).view(-1, 16).max(1).values.to(torch.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=131072)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--recipe-points', type=int, default=64)
    a = ap.parse_args()
    from src.training import NODE_WAN_solver
    d, M = 20, a.points
    params = {'alpha': 1e8, 'u_layers': 8, 'u_hidden_dim': 20, 'u_hidden_hidden_dim': 10, 'v_layers': 9, 'v_hidden_dim': 50,
              'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'dopri5',
              'dim': d, 'N_t': 20, 'N_r': 4000, 'N_b': 4000, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 1,
              'domain': 'Hypercube'}

    def solver(name):
        torch.manual_seed(0)
        return NODE_WAN_solver(dict(params, solver=name), P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g,
                               torch.device('cuda'), './', func_u_sol=P.func_u_sol, p=2)
    S, Sm = solver('dopri5'), solver('midpoint')
    dev = S.device
    g = torch.Generator().manual_seed(1)
    pts = torch.cat((torch.rand(M, 1, generator=g, dtype=F64), torch.rand(M, d, generator=g, dtype=F64) * 2 - 1), 1)
    pts_dev = pts.to(dev)
    out = {'points': M, 'dopri5_stepper_trained': S.engine.dopri5_stepper}

    # 1. evaluate with dopri5 (sorted by t - t_in inside): host points (upload included) and device points; midpoint at N_t beside it
    out['evaluate_dopri5_ms_host_points'] = timed(lambda: S.evaluate(pts), a.reps, 'evaluate_dopri5_ms_host_points')
    out['evaluate_dopri5_ms_device_points'] = timed(lambda: S.evaluate(pts_dev), a.reps, 'evaluate_dopri5_ms_device_points')
    out['evaluate_midpoint_ms_device_points'] = timed(lambda: Sm.evaluate(pts_dev), a.reps, 'evaluate_midpoint_ms_device_points')
    out['max_abs_dopri5_minus_midpoint'] = float((S.evaluate(pts_dev) - Sm.evaluate(pts_dev)).abs().max())

    # 2. the launch chain alone, unsorted and sorted; steps per path and the padded work of the tiles
    net = S.u_net.module
    th, (H, K), m, Hn = net.blob.data, net.kdims, 8, 20
    xT = pts_dev[:, 1:].t().contiguous()
    t_in, t_end = torch.zeros(M, dtype=F64, device=dev), pts_dev[:, 0].contiguous()
    s = P.func_h(torch.cat((t_in.view(M, 1), pts_dev[:, 1:]), 1)).reshape(-1).double().contiguous()
    run = lambda o=None: EP.paths_dopri5(xT if o is None else xT[:, o].contiguous(), t_in, t_end if o is None else t_end[o].contiguous(),   # noqa: E731
                                         s if o is None else s[o].contiguous(), th, H, K, m, Hn, KN.DOPRI5_RTOL, KN.DOPRI5_ATOL)
    order = EP.sort_by_steps(t_end)[0]
    for name, o in (('unsorted', None), ('sorted', order)):
        r = run(o)
        att, acc = r['n_att'].double(), r['n_acc'].double()
        rounds = tile_rounds(r['n_att'])
        out['kernel_ms_' + name] = timed(lambda: run(o), a.reps, 'kernel_ms_' + name)
        out['padded_work_' + name] = float(16 * rounds.sum()) / max(float(att.sum()), 1.0)
        out['tile_rounds_mean_' + name], out['tile_rounds_max_' + name] = float(rounds.double().mean()), int(rounds.max())
    out.update(accepted_mean=float(acc.mean()), accepted_max=int(acc.max()), attempted_mean=float(att.mean()),
               attempted_max=int(att.max()), status_nonzero=int((r['status'] != 0).sum()))

    # 3. one round against kq_attempt's launch: N_r = 4000 paths (250 tiles, at most one per CU), all over the whole interval, so
    #    that every tile walks about the same rounds; the lift and the two field evaluations of the first step are in the time
    Nk = 4000
    xk, sk, zk, ok = xT[:, :Nk].contiguous(), s[:Nk].contiguous(), t_in[:Nk].contiguous(), torch.ones(Nk, dtype=F64, device=dev)
    rk = EP.paths_dopri5(xk, zk, ok, sk, th, H, K, m, Hn, KN.DOPRI5_RTOL, KN.DOPRI5_ATOL)
    ms = timed(lambda: EP.paths_dopri5(xk, zk, ok, sk, th, H, K, m, Hn, KN.DOPRI5_RTOL, KN.DOPRI5_ATOL), a.reps, 'whole_interval_ms')
    rounds = tile_rounds(rk['n_att'])
    out.update(whole_interval_paths=Nk, whole_interval_ms=ms, whole_interval_rounds_max=int(rounds.max()),
               whole_interval_rounds_mean=float(rounds.double().mean()), us_per_round=ms * 1e3 / int(rounds.max()))

    # 4. before: the README recipe with dopri5, one point per call, over a sample of the points
    Q = min(a.recipe_points, M)

    def recipe():
        with torch.no_grad():
            for i in range(Q):
                x0 = pts[i].clone()
                x0[0] = 0.0
                S.u_net(torch.stack((x0, pts[i])).unsqueeze(0))
    out['recipe_points'] = Q
    out['recipe_ms_per_point'] = timed(recipe, max(1, a.reps // 2)) / Q
    out['recipe_s_extrapolated'] = out['recipe_ms_per_point'] * M / 1e3
    out['min_max_ms'] = SPREAD
    print(json.dumps(out))


if __name__ == '__main__':
    main()
