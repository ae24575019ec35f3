"""Cost of second derivatives of u at scattered points (NODE_WAN_solver.evaluate_hvp / evaluate_hess, csrc/xw_tiled_paths_hvp.hip)
against what there was before.  Workload: the YAML network (20, 10, 8) at initialisation, midpoint, N_t = 20, d = 20, M uniform
random points of the cube x [T0, T].  In one process, every route warmed up, then timed alternately, every timed call ended by a
device synchronise:
  evaluate_hvp, evaluate_hess            with the points on the host and on the device
  evaluate_grad                          the first-order chain the new one extends
  central differences                    the route a user had: 2 d evaluate_grad calls at x +- eps e_k, over a SAMPLE of the points
                                         (reported per point and scaled to the cloud), and the accuracy of that quotient against
                                         `hess` at several eps
  the oracle's double backward           per point on the host: autograd's Hessian of x -> refspec.u_net([[T0, x] .. [t, x]], h),
                                         over a smaller sample, reported per point
and, between device synchronises, the launch chain alone: kernels.tiled_paths_hvp per direction next to kernels.tiled_paths_grad
on the same sorted group.
python tools/eval_hess_rate.py [--points M] [--sample S] [--oracle-sample O] [--reps R] [--md FILE]   (one JSON line at the end)"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import configs.Ex4_1_funcs as P                                    # noqa: E402

F64 = torch.float64
EPS = (1e-2, 1e-3, 1e-4, 1e-5, 1e-6)


def once(fn):
    """wall time of one fn() in ms, ended by a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(ts):
    return sorted(ts)[len(ts) // 2]


def central_differences(S, pts, eps):
    """hess [M, d, d] from 2 d evaluate_grad calls: row k = (grad(x + eps e_k) - grad(x - eps e_k)) / (2 eps)"""
    d = pts.shape[1] - 1
    rows = []
    for k in range(d):
        step = torch.zeros_like(pts)
        step[:, 1 + k] = eps
        rows.append((S.evaluate_grad(pts + step)['grad'] - S.evaluate_grad(pts - step)['grad']) / (2 * eps))
    return torch.stack(rows, 1)


def oracle_hessians(S, pts, params):
    """autograd's Hessian of x -> refspec.u_net on the one-path group of every point, on the host: [O, d, d]"""
    from oracle import refspec as R
    named = dict(S.u_net.named_parameters())
    theta = {k: named[nm].detach().cpu().clone() for nm, k in R.u_names(params['u_layers'])}
    T0, T, n_sub = params['T0'], params['T'], params['N_t']
    out = []
    for p in pts:
        t = float(p[0])
        n = 0 if t == T0 else max(1, math.ceil((t - T0) / ((T - T0) / n_sub)))
        grid = torch.tensor([T0 + (t - T0) * k / n for k in range(n)] + [t], dtype=F64)

        def U(x):
            X = torch.cat((grid.view(1, -1, 1), x.view(1, 1, -1).expand(1, n + 1, -1)), 2)
            return R.u_net(theta, params, X, P.func_h(X[:, 0, :]).reshape(-1)).reshape(-1)[-1]
        out.append(torch.autograd.functional.hessian(U, p[1:].clone()))
    return torch.stack(out)


def launch_chain(S, pts_dev, reps):
    """ms of one kernels.tiled_paths_hvp launch (one direction) and of one kernels.tiled_paths_grad launch on the cloud's sorted
    group, checkpoints in place: medians over reps, each between two device synchronises"""
    from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN
    net = S.u_net.module
    dev, (H, K), m = pts_dev.device, net.kdims, net.num_layers
    e = EP.second_order_entry('eval_hess_rate', pts_dev, None, net.setup, net.domain, net.solver, net.h, dev, S.options.eval_chunk_paths)
    L, M, d = e.tT.shape[0], e.M, e.d
    new = lambda *s: torch.empty(*s, dtype=F64, device=dev)           # noqa: E731
    job = dict(xT=e.xT, start=e.start, tT=e.tT, nstep=e.nstep, u=new(L, M), Y=new(L, H, M))
    KN.tiled_paths_fwd([job], net.blob.data, net.method, H, K, m)
    gj = dict(job, gx=new(d, M), gs=new(M))
    hj = dict(job, vx=torch.randn(d, M, dtype=F64, device=dev), vs=torch.randn(M, dtype=F64, device=dev), Yd=new(L, H, M), ju=new(M),
              hx=new(d, M), hs=new(M))
    work = KN.paths_hvp_work(d, H, K, m, (M + 15) // 16, dev)
    fns = {'tiled_paths_grad': lambda: KN.tiled_paths_grad([gj], net.blob.data, net.method, H, K, m),
           'tiled_paths_hvp': lambda: KN.tiled_paths_hvp([hj], net.blob.data, net.method, H, K, m, work=work),
           'tiled_paths_hvp_ju_only': lambda: KN.tiled_paths_hvp([{k: v for k, v in hj.items() if k not in ('hx', 'hs')}], net.blob.data,
                                                                  net.method, H, K, m, work=work)}
    for fn in fns.values():
        fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(once(fn))
    return {k + '_ms': median(v) for k, v in ts.items()}, L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=131072)
    ap.add_argument('--sample', type=int, default=4096, help='points the central differences are timed and compared over')
    ap.add_argument('--oracle-sample', type=int, default=16, help='points the host double backward is timed over')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--md', default=None, help='also write the numbers as a markdown note to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('eval_hess_rate: no GPU visible -- a rate is measured on the device or not at all')
    from src.training import NODE_WAN_solver
    d, M = 20, a.points
    S_, O_ = min(a.sample, M), min(a.oracle_sample, M)
    params = {'alpha': 1e8, 'u_layers': 8, 'u_hidden_dim': 20, 'u_hidden_hidden_dim': 10, 'v_layers': 9, 'v_hidden_dim': 50,
              'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'midpoint',
              'dim': d, 'N_t': 20, 'N_r': 4000, 'N_b': 4000, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 1,
              'domain': 'Hypercube'}
    torch.manual_seed(0)
    S = NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, torch.device('cuda'), './',
                        func_u_sol=P.func_u_sol, p=2)
    g = torch.Generator().manual_seed(1)
    pts = torch.cat((torch.rand(M, 1, generator=g, dtype=F64), torch.rand(M, d, generator=g, dtype=F64) * 2 - 1), 1)
    v = torch.randn(M, d, generator=g, dtype=F64)
    pts_dev, v_dev = pts.to(S.device), v.to(S.device)
    sample_dev = pts_dev[:S_].contiguous()

    fns = {'evaluate_hvp_host_points': lambda: S.evaluate_hvp(pts, v), 'evaluate_hvp_device_points': lambda: S.evaluate_hvp(pts_dev, v_dev),
           'evaluate_hess_host_points': lambda: S.evaluate_hess(pts), 'evaluate_hess_device_points': lambda: S.evaluate_hess(pts_dev),
           'evaluate_grad_host_points': lambda: S.evaluate_grad(pts), 'evaluate_grad_device_points': lambda: S.evaluate_grad(pts_dev),
           'central_differences_sample_device_points': lambda: central_differences(S, sample_dev, 1e-4),
           'evaluate_hess_sample_device_points': lambda: S.evaluate_hess(sample_dev),
           'oracle_double_backward_sample': lambda: oracle_hessians(S, pts[:O_], params)}
    for fn in fns.values():                                          # warm-up of every shape the timed window uses
        fn()
    ts = {k: [] for k in fns}
    for _ in range(a.reps):                                          # alternating: the routes share whatever else the host is doing
        for k, fn in fns.items():
            ts[k].append(once(fn))
    out = {'solver': 'midpoint', 'points': M, 'dim': d, 'sample': S_, 'oracle_sample': O_, 'reps': a.reps}
    for k, t in ts.items():
        out[k + '_ms'] = median(t)
        out[k + '_ms_min_max'] = [min(t), max(t)]
    out['central_differences_ms_for_the_cloud'] = out['central_differences_sample_device_points_ms'] * M / S_
    out['oracle_ms_per_point'] = out['oracle_double_backward_sample_ms'] / O_
    out['oracle_s_for_the_cloud'] = out['oracle_ms_per_point'] * M / 1e3
    out['evaluate_hess_us_per_point'] = out['evaluate_hess_device_points_ms'] * 1e3 / M
    # accuracy: the quotient against hess on the sample, hess against the oracle on its sample; the asymmetry of hess
    hess = S.evaluate_hess(sample_dev)['hess']
    scale = float(hess.abs().max())
    out['hess_scale'] = scale
    out['hess_asymmetry_rel'] = float((hess - hess.transpose(1, 2)).abs().max()) / scale
    out['central_differences_rel_error'] = {'%g' % eps: float((central_differences(S, sample_dev, eps) - hess).abs().max()) / scale
                                            for eps in EPS}
    ref = oracle_hessians(S, pts[:O_], params)
    out['hess_vs_oracle_rel_error'] = float((hess[:O_].cpu() - ref).abs().max()) / float(ref.abs().max())
    chain, L = launch_chain(S, pts_dev, a.reps)
    out.update(chain)
    out['time_levels'] = L
    print(json.dumps(out))
    if a.md:
        with open(a.md, 'w') as f:
            f.write('solver midpoint, %d points, d = %d, %d time levels\n\n| route | median ms | min .. max ms |\n|---|---|---|\n' % (M, d, L))
            for k in fns:
                f.write('| %s | %.3f | %.3f .. %.3f |\n' % (k, out[k + '_ms'], *out[k + '_ms_min_max']))
            f.write('\ncentral differences (2 d evaluate_grad calls, %d points per timed call): %.1f ms scaled to the cloud; oracle double '
                    'backward: %.2f ms per point (%d points per timed call), %.0f s for the cloud; evaluate_hess: %.3f us per point\n'
                    % (S_, out['central_differences_ms_for_the_cloud'], out['oracle_ms_per_point'], O_, out['oracle_s_for_the_cloud'],
                       out['evaluate_hess_us_per_point']))
            f.write('\nlaunch chain on the whole cloud, one direction: tiled_paths_hvp %.3f ms (ju only, the tangent forward alone: %.3f ms); '
                    'tiled_paths_grad %.3f ms\n' % (out['tiled_paths_hvp_ms'], out['tiled_paths_hvp_ju_only_ms'], out['tiled_paths_grad_ms']))
            f.write('\nhess: scale %.3e, asymmetry %.3e of it, against the oracle on %d points %.3e\n\n| eps | central differences against hess, '
                    'relative to scale |\n|---|---|\n' % (scale, out['hess_asymmetry_rel'], O_, out['hess_vs_oracle_rel_error']))
            for eps, err in out['central_differences_rel_error'].items():
                f.write('| %s | %.3e |\n' % (eps, err))


if __name__ == '__main__':
    main()
