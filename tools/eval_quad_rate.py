"""Cost of the second-order forward jets at scattered points (NODE_WAN_solver.evaluate_quad / evaluate_lap / evaluate_residual,
csrc/xw_tiled_paths_jet.hip) against the routes there were before.  Workload: the YAML network (20, 10, 8) at initialisation,
midpoint, N_t = 20, d = 20, M uniform random points of the cube x [T0, T], the points on the device.  In one process, every route
warmed up, then timed alternately, every timed call ended by a device synchronise:
  evaluate_lap                           the Laplacian: d unit directions in one launch per chunk
  evaluate_quad, R = 1 and R = 20        random directions per point
  evaluate_residual                      evaluate_grad + evaluate_lap with Ex4_1's coefficients tabulated on the points
  evaluate_hess, evaluate_hvp,           the forward-over-reverse chain (d launch chains, the [M, d, d] output) and the first-order
  evaluate_grad                          chain, in the same run
and the largest deviation of evaluate_lap's `lap` from evaluate_hess()['lap'], relative to the latter's scale; between device
synchronises, the launches alone: kernels.tiled_paths_jet with R = 1 and, in evaluate_lap's chunks, R = d on the cloud's sorted group.
python tools/eval_quad_rate.py [--points M] [--reps R] [--md FILE]   (one JSON line at the end)"""
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


def launch_alone(S, pts_dev, reps):
    """ms of the kernels.tiled_paths_jet launches alone on the cloud's sorted group, directions in place: R = 1 in one launch, R = d
    in evaluate_lap's chunks (evalpaths.jet_chunk_paths at R = d); medians over reps, each between two device synchronises; and
    the chunk's paths"""
    from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN
    net = S.u_net.module
    dev, (H, K), m = pts_dev.device, net.kdims, net.num_layers
    e = EP.second_order_entry('eval_quad_rate', pts_dev, None, net.setup, net.domain, net.solver, net.h, dev, S.options.eval_chunk_paths)
    d, M = e.d, e.M
    k = min(M, EP.jet_chunk_paths(S.options.eval_chunk_paths, d, KN.lib.xw_paths_tiled_jet_work(d, H, K, m)))
    new = lambda *s: torch.empty(*s, dtype=F64, device=dev)           # noqa: E731

    def jobs_of(R, per):
        out = []
        for lo in range(0, M, per):
            n = min(lo + per, M) - lo
            out.append(dict(xT=e.xT[:, lo:lo + n].contiguous(), start=e.start[lo:lo + n], tT=e.tT[:, lo:lo + n].contiguous(),
                            nstep=e.nstep[lo:lo + n], vx=torch.randn(R, d, n, dtype=F64, device=dev),
                            vs=torch.randn(R, n, dtype=F64, device=dev), qs=torch.randn(R, n, dtype=F64, device=dev), u=new(n),
                            ju=new(R, n), quu=new(R, n)))
        return out

    def launcher(R, per):                                            # (the launches of a route share the stream and the workspace)
        jobs = jobs_of(R, per)
        work = KN.paths_jet_work(d, H, K, m, R * ((min(per, M) + 15) // 16), dev)

        def run():
            for job in jobs:
                n = job['xT'].shape[1]
                KN.tiled_paths_jet([job], net.blob.data, net.method, H, K, m, work=work[:work.numel() // ((min(per, M) + 15) // 16) * ((n + 15) // 16)])
        return run
    fns = {'tiled_paths_jet_R1': launcher(1, M), 'tiled_paths_jet_R%d' % d: launcher(d, k)}
    for fn in fns.values():
        fn()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ts[name].append(once(fn))
    return {name + '_ms': median(v) for name, v in ts.items()}, k, e.tT.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=131072)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--md', default=None, help='also write the numbers as a markdown note to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('eval_quad_rate: no GPU visible -- a rate is measured on the device or not at all')
    from src.training import NODE_WAN_solver
    d, M = 20, a.points
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
    V1 = v_dev.view(M, 1, d)
    Vd = torch.randn(M, d, d, generator=torch.Generator(device=S.device).manual_seed(2), dtype=F64, device=S.device)

    fns = {'evaluate_lap': lambda: S.evaluate_lap(pts_dev), 'evaluate_quad_R1': lambda: S.evaluate_quad(pts_dev, V1),
           'evaluate_quad_R%d' % d: lambda: S.evaluate_quad(pts_dev, Vd), 'evaluate_residual': lambda: S.evaluate_residual(pts_dev),
           'evaluate_hess': lambda: S.evaluate_hess(pts_dev), 'evaluate_hvp': lambda: S.evaluate_hvp(pts_dev, v_dev),
           'evaluate_grad': lambda: S.evaluate_grad(pts_dev)}
    for fn in fns.values():                                          # warm-up of every shape the timed window uses
        fn()
    ts = {k: [] for k in fns}
    for _ in range(a.reps):                                          # alternating: the routes share whatever else the host is doing
        for k, fn in fns.items():
            ts[k].append(once(fn))
    out = {'solver': 'midpoint', 'points': M, 'dim': d, 'reps': a.reps, 'points_on': 'device'}
    for k, t in ts.items():
        out[k + '_ms'] = median(t)
        out[k + '_ms_min_max'] = [min(t), max(t)]
    out['evaluate_lap_us_per_point'] = out['evaluate_lap_ms'] * 1e3 / M
    out['evaluate_hess_over_evaluate_lap'] = out['evaluate_hess_ms'] / out['evaluate_lap_ms']
    lap, hess = S.evaluate_lap(pts_dev), S.evaluate_hess(pts_dev)
    scale = float(hess['lap'].abs().max())
    out['lap_scale'] = scale
    out['lap_vs_evaluate_hess_rel'] = float((lap['lap'] - hess['lap']).abs().max()) / scale
    out['u_bits_of_evaluate'] = bool(torch.equal(lap['u'], S.evaluate(pts_dev)))
    del hess
    q = S.evaluate_quad(pts_dev, V1)
    hv = S.evaluate_hvp(pts_dev, v_dev)
    want = (hv['hvp'] * v_dev).sum(1)
    out['quad_vs_v_dot_hvp_rel'] = float((q['quad'][:, 0] - want).abs().max()) / float(want.abs().max())
    out['residual_abs_max'] = float(S.evaluate_residual(pts_dev)['residual'].abs().max())
    alone, k, L = launch_alone(S, pts_dev, a.reps)
    out.update(alone)
    out['launch_alone_paths'], out['time_levels'] = k, L
    print(json.dumps(out))
    if a.md:
        with open(a.md, 'w') as f:
            f.write('solver midpoint, %d points on the device, d = %d, %d time levels\n\n| route | median ms | min .. max ms |\n|---|---|---|\n'
                    % (M, d, L))
            for name in fns:
                f.write('| %s | %.3f | %.3f .. %.3f |\n' % (name, out[name + '_ms'], *out[name + '_ms_min_max']))
            f.write('\nevaluate_lap: %.3f us per point; evaluate_hess / evaluate_lap = %.2f\n'
                    % (out['evaluate_lap_us_per_point'], out['evaluate_hess_over_evaluate_lap']))
            f.write('\nlap against evaluate_hess()[\'lap\']: largest deviation %.3e of its scale %.3e; quad (R = 1) against v . hvp: %.3e; '
                    'u has the bits of evaluate: %s; largest |residual| at initialisation %.3e\n'
                    % (out['lap_vs_evaluate_hess_rel'], scale, out['quad_vs_v_dot_hvp_rel'], out['u_bits_of_evaluate'], out['residual_abs_max']))
            f.write('\nthe launches alone on the whole cloud: tiled_paths_jet R = 1, one launch, %.3f ms; R = %d in chunks of %d paths %.3f ms\n'
                    % (out['tiled_paths_jet_R1_ms'], d, k, out['tiled_paths_jet_R%d_ms' % d]))


if __name__ == '__main__':
    main()
