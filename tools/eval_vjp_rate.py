"""Cost of the parameter gradients of u at scattered points (NODE_WAN_solver.evaluate_vjp, csrc/xw_tiled_paths_vjp.hip) next to
evaluate_grad and evaluate in the same process, and against the routes there were before.  Workload: the YAML network (20, 10, 8) at
initialisation, midpoint, N_t = 20, d = 20, M uniform random points of the cube x [T0, T], on the device.  Every route is warmed up,
then the routes are timed alternately, every timed call ended by a device synchronise:
  evaluate_vjp / evaluate_grad / evaluate   the three public calls on the same cloud
  sweep_vjp / sweep_grad                    one launch of kernels.tiled_paths_vjp (its slabs' zeroing included) and of
                                            kernels.tiled_paths_grad (gx, gs) over the same checkpoints: the sorted cloud's first chunk
  shared_grid                               the same number of points on ONE grid of mean-step-count steps through the existing
                                            u_net(X[N, L, d + 1]).sum().backward(): what a group without raggedness costs; the
                                            path-steps of both are reported, a tile of the ragged group walking its longest path's
  host_sample                               oracle.refspec.u_net(...).backward() per point over a sample, reported per point
python tools/eval_vjp_rate.py [--points M] [--sample S] [--reps R] [--md FILE]   (one JSON line at the end)"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import configs.Ex4_1_funcs as P                                    # noqa: E402

F64 = torch.float64


def once(fn):
    """wall time of one fn() in ms, ended by a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(ts):
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=131072)
    ap.add_argument('--sample', type=int, default=64, help='points the host route is timed over')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--md', default=None, help='also write the numbers as a markdown note to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('eval_vjp_rate: no GPU visible -- a rate is measured on the device or not at all')
    from oracle import refspec as R
    from src.training import NODE_WAN_solver
    from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN
    d, M, S_ = 20, a.points, min(a.sample, a.points)
    params = {'alpha': 1e8, 'u_layers': 8, 'u_hidden_dim': 20, 'u_hidden_hidden_dim': 10, 'v_layers': 9, 'v_hidden_dim': 50,
              'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'midpoint',
              'dim': d, 'N_t': 20, 'N_r': 4000, 'N_b': 4000, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 1,
              'domain': 'Hypercube'}
    torch.manual_seed(0)
    S = NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, torch.device('cuda'), './',
                        func_u_sol=P.func_u_sol, p=2)
    net, dev = S.u_net.module, S.device
    g = torch.Generator().manual_seed(1)
    pts = torch.cat((torch.rand(M, 1, generator=g, dtype=F64), torch.rand(M, d, generator=g, dtype=F64) * 2 - 1), 1)
    w = torch.randn(M, generator=g, dtype=F64).to(dev)
    pts_dev = pts.to(dev)

    # one chunk of the sorted cloud, as evaluate_points_vjp packs it: the two sweeps over the same checkpoints
    H, K, m, mid, theta = net.kdims[0], net.kdims[1], net.num_layers, net.method, net.blob.data
    t = pts_dev[:, 0].contiguous()
    n = EP.step_counts(t, torch.zeros_like(t), 0, 1, params['N_t'])
    order, _ = EP.sort_by_steps(n)
    L = int(n.max()) + 1
    per = EP.vjp_chunk_paths(S.options.eval_chunk_paths, L, H, theta.numel())
    k = min(per, M)
    sel = order[:k]
    new = lambda *shape: torch.empty(*shape, dtype=F64, device=dev)   # noqa: E731
    zero = torch.zeros(k, dtype=F64, device=dev)
    tT = EP.pack_grids(t[sel], zero, n[sel])
    job = dict(xT=pts_dev[sel, 1:].t().contiguous(), start=P.func_h(torch.cat((zero.view(-1, 1), pts_dev[sel, 1:]), 1)).reshape(-1).double(),
               tT=tT, nstep=n[sel].to(torch.int32), u=new(tT.shape[0], k), Y=new(tT.shape[0], H, k))
    KN.tiled_paths_fwd([job], theta, mid, H, K, m)
    vj = dict(job, w=w[sel].contiguous(), gslab=new((k + 15) // 16, theta.numel()), gx=new(d, k), gs=new(k))
    gj = dict(job, gx=new(d, k), gs=new(k))
    work = KN.paths_vjp_work(d, H, K, m, (k + 15) // 16, dev)

    # the same number of points on one grid
    Ls = int(round(float(n.double().mean()))) + 1
    X = pts_dev.unsqueeze(1).repeat(1, Ls, 1)
    X[:, :, 0] = torch.linspace(0, 1, Ls, dtype=F64, device=dev).view(1, -1)

    def shared_grid():
        for p in net.parameters():
            p.grad = None
        net(X, starts_at_T0=True).sum().backward()

    th_host = {key: dict(net.named_parameters())[name[len('module.'):]].detach().cpu().clone().requires_grad_(True) for name, key in R.u_names(m)}

    n_host = EP.step_counts(pts[:S_, 0], torch.zeros(S_, dtype=F64), 0, 1, params['N_t'])
    grids = EP.pack_grids(pts[:S_, 0].contiguous(), torch.zeros(S_, dtype=F64), n_host)

    def host_sample():
        for i in range(S_):
            ni = int(n_host[i])
            Xi = torch.cat((grids[:ni + 1, i].view(1, -1, 1), pts[i, 1:].view(1, 1, -1).expand(1, ni + 1, -1)), 2)
            R.u_net(th_host, params, Xi, P.func_h(Xi[:, 0, :]).reshape(-1)).reshape(-1)[-1].backward()

    fns = {'evaluate_vjp': lambda: S.evaluate_vjp(pts_dev, w), 'evaluate_grad': lambda: S.evaluate_grad(pts_dev),
           'evaluate': lambda: S.evaluate(pts_dev),
           'sweep_vjp': lambda: KN.tiled_paths_vjp([vj], theta, mid, H, K, m, work=work),
           'sweep_grad': lambda: KN.tiled_paths_grad([gj], theta, mid, H, K, m),
           'shared_grid': shared_grid, 'host_sample': host_sample}
    for fn in fns.values():                                          # warm-up of every shape the timed window uses
        fn()
    ts = {key: [] for key in fns}
    for _ in range(a.reps):                                          # alternating: the routes share whatever else the host is doing
        for key, fn in fns.items():
            ts[key].append(once(fn))
    ns = n[sel].view(-1).cpu()
    tile_steps = int(sum(int(ns[lo:lo + 16].max()) * 16 for lo in range(0, k, 16)))
    out = {'points': M, 'sample': S_, 'reps': a.reps, 'family_trained': S.engine.stepper, 'chunk_paths': per, 'sweep_paths': k,
           'sweep_path_steps': tile_steps, 'cloud_path_steps': int(n.sum()), 'shared_grid_L': Ls, 'shared_grid_path_steps': M * (Ls - 1)}
    for key, v in ts.items():
        out[key + '_ms'] = median(v)
        out[key + '_ms_min_max'] = [min(v), max(v)]
    out['host_ms_per_point'] = out['host_sample_ms'] / S_
    out['evaluate_vjp_us_per_point'] = out['evaluate_vjp_ms'] * 1e3 / M
    out['sweep_vjp_over_grad'] = out['sweep_vjp_ms'] / out['sweep_grad_ms']
    print(json.dumps(out))
    if a.md:
        with open(a.md, 'w') as f:
            f.write('midpoint, (20, 10, 8), d = 20, %d points on the device\n\n| route | median ms | min .. max ms |\n|---|---|---|\n' % M)
            for key in fns:
                f.write('| %s | %.3f | %.3f .. %.3f |\n' % (key, out[key + '_ms'], *out[key + '_ms_min_max']))
            f.write('\nevaluate_vjp: %.3f us per point; host route: %.3f ms per point (%d points per timed call)\n'
                    % (out['evaluate_vjp_us_per_point'], out['host_ms_per_point'], S_))
            f.write('sweeps: %d paths of the sorted cloud (chunk bound %d), %d path-steps walked; vjp / grad = %.2f\n'
                    % (k, per, tile_steps, out['sweep_vjp_over_grad']))
            f.write('cloud: %d path-steps; shared grid: L = %d, %d path-steps\n' % (out['cloud_path_steps'], Ls, out['shared_grid_path_steps']))


if __name__ == '__main__':
    main()
