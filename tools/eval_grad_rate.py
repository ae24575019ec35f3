"""Cost of u, its x-gradient and its time derivative at scattered points (NODE_WAN_solver.evaluate_grad,
csrc/xw_tiled_paths_grad.hip) against the route there was before: the README recipe with autograd, one
u_net([[x0, x]]).sum().backward() per point, X.grad read back.  Workload: the YAML network (20, 10, 8) at initialisation, midpoint,
N_t = 20, d = 20, M uniform random points of the cube x [T0, T].  Both routes are warmed up, then timed alternately, every timed
call ended by a device synchronise; the recipe runs over a sample of the points and is reported per point.
--solver dopri5: the same network and cloud with the adaptive solver (csrc/xw_tdopri_paths.hip, csrc/xw_tdopri_paths_grad.hip), and, in
a call of its own after the timed window (its synchronises slow the chain), where one evaluate_grad spends its time: pass 1,
evalpaths.paths_dopri5 (u, status, step counts); pass 3, the launches of the second forward and the sweep; pass 2, what
evalpaths.dopri5_grad_pass does around those launches (the sort by step count, the gathers, the chunking, the allocations); and the
host side around the passes (entry rule, h and dh/dx by autograd, uploads, the gather back).
python tools/eval_grad_rate.py [--solver midpoint|dopri5] [--points M] [--sample S] [--reps R] [--md FILE]   (one JSON line at the end)"""
import argparse
import json
import os
import sys
import time
from unittest import mock

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


def dopri5_passes(S, pts):
    """ms of one S.evaluate_grad(pts) with solver 'dopri5' and of its passes (module docstring), every timed piece between two device
    synchronises; and the accepted step counts of the cloud"""
    from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN
    ms = dict(total=0.0, pass1=0.0, grad_pass=0.0, pass3=0.0)
    seen = {}

    def timed(fn, key):
        def wrapped(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **kw)
            torch.cuda.synchronize()
            ms[key] += (time.perf_counter() - t0) * 1e3
            return r
        return wrapped
    fwd, first = KN.paths_dopri5_fwd, EP.paths_dopri5

    def second_forward(jobs, *a, **kw):                              # (pass 1 goes through the same wrapper, without checkpoints)
        return (timed(fwd, 'pass3') if jobs[0].get('ckpt') is not None else fwd)(jobs, *a, **kw)

    def first_pass(*a, **kw):
        seen['r'] = timed(first, 'pass1')(*a, **kw)
        return seen['r']
    with mock.patch.object(EP, 'paths_dopri5', first_pass), mock.patch.object(EP, 'dopri5_grad_pass', timed(EP.dopri5_grad_pass, 'grad_pass')), \
            mock.patch.object(KN, 'paths_dopri5_fwd', second_forward), \
            mock.patch.object(KN, 'paths_dopri5_grad', timed(KN.paths_dopri5_grad, 'pass3')):
        timed(S.evaluate_grad, 'total')(pts)
    n_acc = seen['r']['n_acc']
    return dict(total_ms=ms['total'], pass1_ms=ms['pass1'], pass2_ms=ms['grad_pass'] - ms['pass3'], pass3_ms=ms['pass3'],
                host_ms=ms['total'] - ms['pass1'] - ms['grad_pass'],
                n_acc_min_median_max=[int(n_acc.min()), int(n_acc.median()), int(n_acc.max())],
                chunks=EP.dopri5_grad_chunks(n_acc.sort().values.tolist(), S.u_net.module.kdims[0], S.options.eval_chunk_paths))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--solver', choices=('midpoint', 'dopri5'), default='midpoint')
    ap.add_argument('--points', type=int, default=131072)
    ap.add_argument('--sample', type=int, default=256, help='points the per-point recipe is timed over')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--md', default=None, help='also write the numbers as a markdown note to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('eval_grad_rate: no GPU visible -- a rate is measured on the device or not at all')
    from src.training import NODE_WAN_solver
    d, M, S_ = 20, a.points, min(a.sample, a.points)
    params = {'alpha': 1e8, 'u_layers': 8, 'u_hidden_dim': 20, 'u_hidden_hidden_dim': 10, 'v_layers': 9, 'v_hidden_dim': 50,
              'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': a.solver,
              'dim': d, 'N_t': 20, 'N_r': 4000, 'N_b': 4000, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 1,
              'domain': 'Hypercube'}
    torch.manual_seed(0)
    S = NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, torch.device('cuda'), './',
                        func_u_sol=P.func_u_sol, p=2)
    g = torch.Generator().manual_seed(1)
    pts = torch.cat((torch.rand(M, 1, generator=g, dtype=F64), torch.rand(M, d, generator=g, dtype=F64) * 2 - 1), 1)
    pts_dev = pts.to(S.device)

    def recipe():
        """per point: the shared-grid group [[x0, x]], backward, X.grad -- row 1 holds du/d(t, x) at the point"""
        out = []
        for i in range(S_):
            x0 = pts[i].clone()
            x0[0] = 0.0
            X = torch.stack((x0, pts[i])).unsqueeze(0).requires_grad_(True)
            S.u_net(X).sum().backward()
            out.append(X.grad)
        return out

    fns = {'evaluate_grad_host_points': lambda: S.evaluate_grad(pts), 'evaluate_grad_device_points': lambda: S.evaluate_grad(pts_dev),
           'evaluate_host_points': lambda: S.evaluate(pts), 'evaluate_device_points': lambda: S.evaluate(pts_dev),
           'recipe_sample': recipe}
    for fn in fns.values():                                          # warm-up of every shape the timed window uses
        fn()
    ts = {k: [] for k in fns}
    for _ in range(a.reps):                                          # alternating: the routes share whatever else the host is doing
        for k, fn in fns.items():
            ts[k].append(once(fn))
    out = {'solver': a.solver, 'points': M, 'sample': S_, 'reps': a.reps, 'family_trained': S.engine.stepper}
    for k, v in ts.items():
        out[k + '_ms'] = median(v)
        out[k + '_ms_min_max'] = [min(v), max(v)]
    out['recipe_ms_per_point'] = out['recipe_sample_ms'] / S_
    out['evaluate_grad_us_per_point'] = out['evaluate_grad_host_points_ms'] * 1e3 / M
    out['recipe_s_for_the_cloud'] = out['recipe_ms_per_point'] * M / 1e3
    if a.solver == 'dopri5':
        out['passes_device_points'] = dopri5_passes(S, pts_dev)
        out['passes_host_points'] = dopri5_passes(S, pts)
    print(json.dumps(out))
    if a.md:
        with open(a.md, 'w') as f:
            f.write('solver %s, %d points\n\n| route | median ms | min .. max ms |\n|---|---|---|\n' % (a.solver, M))
            for k in fns:
                f.write('| %s | %.3f | %.3f .. %.3f |\n' % (k, out[k + '_ms'], *out[k + '_ms_min_max']))
            f.write('\nrecipe: %.4f ms per point (%d points per timed call), %.1f s for %d points; evaluate_grad: %.3f us per point\n'
                    % (out['recipe_ms_per_point'], S_, out['recipe_s_for_the_cloud'], M, out['evaluate_grad_us_per_point']))
            for k in ('passes_device_points', 'passes_host_points'):
                if k in out:
                    p = out[k]
                    f.write('\n%s, one call with a synchronise behind every piece: %.1f ms = pass 1 %.1f + pass 2 %.1f + pass 3 %.1f + '
                            'host side %.1f; accepted steps min / median / max %s; chunks (lo, hi, cap) %s\n'
                            % (k, p['total_ms'], p['pass1_ms'], p['pass2_ms'], p['pass3_ms'], p['host_ms'], p['n_acc_min_median_max'],
                               p['chunks']))


if __name__ == '__main__':
    main()
