"""Cost of the parameter gradients of u, du/dx and ut at scattered points (NODE_WAN_solver.evaluate_grad_vjp,
csrc/xw_tiled_paths_gvjp.hip) next to its natural yardstick -- evaluate_vjp + evaluate_hvp + evaluate_grad in the same process -- and
against the one route a user had before: a central difference of two evaluate_vjp calls at x +- eps wg.  Workload: the YAML network
(20, 10, 8) at initialisation, midpoint, N_t = 20, d = 20, M uniform random points of the cube x [T0, T], on the device.  Every
route is warmed up, then the routes are timed alternately, every timed call ended by a device synchronise:
  evaluate_grad_vjp                            all three weights
  evaluate_vjp / evaluate_hvp / evaluate_grad  the three public calls on the same cloud; their sum is the yardstick
  sweep_gvjp / sweep_vjp / sweep_hvp           one launch of kernels.tiled_paths_gvjp, of kernels.tiled_paths_vjp (both with their
                                               slabs' zeroing) and of kernels.tiled_paths_hvp's reverse sweep with its tangent
                                               forward over the same checkpoints: the sorted cloud's first chunk
  central_difference                           (evaluate_vjp(x + eps wg, 1) - evaluate_vjp(x - eps wg, 1)) / (2 eps), the gradient
                                               term alone; its error against evaluate_grad_vjp(wg=wg) per eps, relative to the
                                               block's largest entry -- the start value h([T0, x]) moves with the point, as the
                                               direction (wg, dh/dx . wg) does to first order, and the points cross ReLU kinks
  host_sample                                  autograd through oracle.refspec per point over a sample (create_graph in x, then
                                               theta), reported per point
python tools/eval_grad_vjp_rate.py [--points M] [--sample S] [--reps R] [--md FILE]   (one JSON line at the end)"""
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
    ap.add_argument('--sample', type=int, default=32, help='points the host route is timed over')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--md', default=None, help='also write the numbers as a markdown note to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('eval_grad_vjp_rate: no GPU visible -- a rate is measured on the device or not at all')
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
    pts = torch.cat((torch.rand(M, 1, generator=g, dtype=F64), torch.rand(M, d, generator=g, dtype=F64) * 1.8 - 0.9), 1)
    wu, wt = torch.randn(M, generator=g, dtype=F64).to(dev), torch.randn(M, generator=g, dtype=F64).to(dev)
    wg_host = torch.randn(M, d, generator=g, dtype=F64)
    wg_host = wg_host / wg_host.norm(dim=1, keepdim=True)
    wg, pts_dev = wg_host.to(dev), pts.to(dev)
    ones = torch.ones(M, dtype=F64, device=dev)

    # one chunk of the sorted cloud, as evaluate_points_grad_vjp packs it: the sweeps over the same checkpoints
    H, K, m, mid, theta = net.kdims[0], net.kdims[1], net.num_layers, net.method, net.blob.data
    t = pts_dev[:, 0].contiguous()
    n = EP.step_counts(t, torch.zeros_like(t), 0, 1, params['N_t'])
    order, _ = EP.sort_by_steps(n)
    L = int(n.max()) + 1
    per = EP.gvjp_chunk_paths(S.options.eval_chunk_paths, L, H, theta.numel())
    k = min(per, M)
    sel = order[:k]
    tiles = (k + 15) // 16
    new = lambda *shape: torch.empty(*shape, dtype=F64, device=dev)   # noqa: E731
    zero = torch.zeros(k, dtype=F64, device=dev)
    tT = EP.pack_grids(t[sel], zero, n[sel])
    first = torch.cat((zero.view(-1, 1), pts_dev[sel, 1:]), 1)
    job = dict(xT=pts_dev[sel, 1:].t().contiguous(), start=P.func_h(first).reshape(-1).double(), tT=tT, nstep=n[sel].to(torch.int32),
               u=new(tT.shape[0], k), Y=new(tT.shape[0], H, k))
    KN.tiled_paths_fwd([job], theta, mid, H, K, m)
    dirn = dict(vx=wg[sel].t().contiguous(), vs=(EP.start_gradient(P.func_h, first).to(dev) * wg[sel]).sum(1).contiguous(),
                Yd=new(tT.shape[0], H, k))
    hj = dict(job, ju=new(k), hx=new(d, k), hs=new(k), **dirn)
    KN.tiled_paths_hvp([hj], theta, mid, H, K, m)
    gj = dict(job, wu=wu[sel].contiguous(), wt=wt[sel].contiguous(), gslab=new(tiles, theta.numel()), **dirn)
    vj = dict(job, w=wu[sel].contiguous(), gslab=new(tiles, theta.numel()))
    works = (KN.paths_gvjp_work(d, H, K, m, tiles, dev), KN.paths_vjp_work(d, H, K, m, tiles, dev), KN.paths_hvp_work(d, H, K, m, tiles, dev))

    th_host = {key: dict(net.named_parameters())[name[len('module.'):]].detach().cpu().clone().requires_grad_(True) for name, key in R.u_names(m)}
    n_host = EP.step_counts(pts[:S_, 0], torch.zeros(S_, dtype=F64), 0, 1, params['N_t'])
    grids = EP.pack_grids(pts[:S_, 0].contiguous(), torch.zeros(S_, dtype=F64), n_host)

    def host_sample():
        for i in range(S_):
            ni = int(n_host[i])
            x = pts[i, 1:].clone().requires_grad_(True)
            Xi = torch.cat((grids[:ni + 1, i].view(1, -1, 1), x.view(1, 1, -1).expand(1, ni + 1, -1)), 2)
            ui = R.u_net(th_host, params, Xi, P.func_h(Xi[:, 0, :]).reshape(-1)).reshape(-1)[-1]
            gi, = torch.autograd.grad(ui, x, create_graph=True)
            (ui + (gi * wg_host[i]).sum()).backward()

    def central(eps):
        shift = torch.cat((torch.zeros(M, 1, dtype=F64, device=dev), eps * wg), 1)
        hi, lo = S.evaluate_vjp(pts_dev + shift, ones)['params'], S.evaluate_vjp(pts_dev - shift, ones)['params']
        return {key: (hi[key] - lo[key]) / (2 * eps) for key in hi}

    fns = {'evaluate_grad_vjp': lambda: S.evaluate_grad_vjp(pts_dev, wu, wg, wt), 'evaluate_vjp': lambda: S.evaluate_vjp(pts_dev, wu),
           'evaluate_hvp': lambda: S.evaluate_hvp(pts_dev, wg), 'evaluate_grad': lambda: S.evaluate_grad(pts_dev),
           'sweep_gvjp': lambda: KN.tiled_paths_gvjp([gj], theta, mid, H, K, m, work=works[0]),
           'sweep_vjp': lambda: KN.tiled_paths_vjp([vj], theta, mid, H, K, m, work=works[1]),
           'sweep_hvp': lambda: KN.tiled_paths_hvp([hj], theta, mid, H, K, m, work=works[2]),
           'central_difference': lambda: central(1e-4), 'host_sample': host_sample}
    for fn in fns.values():                                          # warm-up of every shape the timed window uses
        fn()
    ts = {key: [] for key in fns}
    for _ in range(a.reps):                                          # alternating: the routes share whatever else the host is doing
        for key, fn in fns.items():
            ts[key].append(once(fn))
    # the central difference's error, the gradient's weight alone, per eps: worst block, relative to the block's largest entry
    exact = S.evaluate_grad_vjp(pts_dev, wg=wg)['params']
    cd_err = {}
    for eps in (1e-2, 1e-3, 1e-4, 1e-5, 1e-6):
        cd = central(eps)
        cd_err['%g' % eps] = max(float((cd[key] - exact[key]).abs().max()) / float(exact[key].abs().max())
                                 for key in exact if float(exact[key].abs().max()) > 0)
    out = {'points': M, 'sample': S_, 'reps': a.reps, 'family_trained': S.engine.stepper, 'chunk_paths': per, 'sweep_paths': k,
           'cloud_path_steps': int(n.sum()), 'central_difference_rel_err': cd_err}
    for key, v in ts.items():
        out[key + '_ms'] = median(v)
        out[key + '_ms_min_max'] = [min(v), max(v)]
    out['yardstick_ms'] = out['evaluate_vjp_ms'] + out['evaluate_hvp_ms'] + out['evaluate_grad_ms']
    out['host_ms_per_point'] = out['host_sample_ms'] / S_
    out['evaluate_grad_vjp_us_per_point'] = out['evaluate_grad_vjp_ms'] * 1e3 / M
    out['sweep_gvjp_over_vjp_plus_hvp'] = out['sweep_gvjp_ms'] / (out['sweep_vjp_ms'] + out['sweep_hvp_ms'])
    print(json.dumps(out))
    if a.md:
        with open(a.md, 'w') as f:
            f.write('midpoint, (20, 10, 8), d = 20, %d points on the device\n\n| route | median ms | min .. max ms |\n|---|---|---|\n' % M)
            for key in fns:
                f.write('| %s | %.3f | %.3f .. %.3f |\n' % (key, out[key + '_ms'], *out[key + '_ms_min_max']))
            f.write('\nevaluate_grad_vjp: %.3f us per point; evaluate_vjp + evaluate_hvp + evaluate_grad: %.3f ms\n'
                    % (out['evaluate_grad_vjp_us_per_point'], out['yardstick_ms']))
            f.write('host route: %.3f ms per point (%d points per timed call)\n' % (out['host_ms_per_point'], S_))
            f.write('sweeps: %d paths of the sorted cloud (chunk bound %d); gvjp / (vjp + hvp) = %.2f\n'
                    % (k, per, out['sweep_gvjp_over_vjp_plus_hvp']))
            f.write('central difference of evaluate_vjp at x +- eps wg (|wg| = 1), worst block error relative to the block\'s scale: '
                    + ', '.join('eps %s: %.2e' % kv for kv in cd_err.items()) + '\n')


if __name__ == '__main__':
    main()
