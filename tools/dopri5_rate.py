"""solver 'dopri5' at the headline shape: what one u_theta forward + sweep costs with the adaptive stepper against midpoint.

Shape: cube, d = 20, two groups of 4096 paths (the interior sample u is integrated on and the boundary sample) sharing one
sorted N_t = 32 grid, the YAML network (u_hidden_dim 20, u_hidden_hidden_dim 10, u_layers 8) or --shape H,K,m, Xavier weights
with zero biases as at initialisation.  The dopri5 forward is one launch pair (init) plus chunks of attempt launches for both
jobs, the sweep one launch with parameter and x gradients (the generator's fused form) -- the stepper part of a dopri5 generator
sub-step, measured through kernels.dopri5_fwd / dopri5_sweep.

--stepper vector (default; csrc/xw_dopri.hip), tiled (csrc/xw_tdopri.hip) or both: the two implementations alternately in ONE
process, each with the median, the smallest and the largest of its repetitions.  midpoint runs on the family that serves the
shape (the fused container, or the tiled family beyond (64, 16) -- where 'vector' does not exist).

    python tools/dopri5_rate.py [--reps 5] [--stepper both] [--shape 128,64,8] [--out profiles/dopri5_rate.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xnode_wan_pde_solver_amd import kernels as KN, nets  # noqa: E402

F64 = torch.float64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--stepper', default='vector', choices=('vector', 'tiled', 'both'),
                    help="dopri5's implementation (kernels.DOPRI5_STEPPERS); both: the two alternately in one process")
    ap.add_argument('--shape', default='20,10,8', help='H,K,m: u_hidden_dim, u_hidden_hidden_dim, u_layers')
    a = ap.parse_args()
    H, K, m = (int(v) for v in a.shape.split(','))
    d, N, L = 20, 4096, 32
    steppers = list(KN.DOPRI5_STEPPERS) if a.stepper == 'both' else [a.stepper]
    torch.manual_seed(0)
    net = nets.XNODE(H, 1, None, None, {'dim': d}, K, m, None, solver='dopri5')
    net.dopri5_stepper = 'tiled' if 'tiled' in steppers else 'vector'
    blob = net.bind(torch.device('cuda')).data
    Hc, Kc = net.kdims
    if net.family == 'tiled' and 'vector' in steppers:
        raise SystemExit("--shape %s is beyond the vector implementation's widths %s: --stepper tiled" % (a.shape, KN.GENERIC_ODE_MAX))
    g = torch.Generator().manual_seed(1)
    t, _ = torch.sort(torch.rand(L, generator=g, dtype=F64))
    t[0], t[-1] = 0.0, 1.0
    t = t.cuda()
    jobs = []
    for _ in range(2):
        xT = (torch.rand(d, N, generator=g, dtype=F64) * 2 - 1).cuda()
        s = torch.randn(N, generator=g, dtype=F64).cuda()
        jobs.append(dict(xT=xT, start=s, u=torch.empty(L, N, dtype=F64, device='cuda'),
                         Y=torch.empty(L, Hc, N, dtype=F64, device='cuda'), ubar=torch.ones(L, N, dtype=F64, device='cuda'),
                         gx=torch.empty(d, N, dtype=F64, device='cuda'), gs=torch.empty(N, dtype=F64, device='cuda'),
                         gslab=torch.empty(KN.ode_bwd_slabs(N), KN.theta_size(d, Hc, Kc), dtype=F64, device='cuda')))
    fwd_jobs = [dict(xT=j['xT'], start=j['start'], u=j['u']) for j in jobs]

    def dopri(stepper):
        t0 = time.perf_counter()
        recs = KN.dopri5_fwd(fwd_jobs, t, blob, Hc, Kc, m, H, stepper=stepper)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        KN.dopri5_sweep([dict(j, rec=r) for j, r in zip(jobs, recs)], t, blob, Hc, Kc, m, want_x=True, want_params=True,
                        x_cot_ones=True, stepper=stepper)
        torch.cuda.synchronize()
        return recs, (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    mid_fwd, mid_bwd = (KN.tiled_ode_fwd_multi, KN.tiled_ode_bwd_multi) if net.family == 'tiled' else (KN.ode_fwd_multi, KN.ode_bwd_multi)

    def midpoint():
        t0 = time.perf_counter()
        mid_fwd([dict(xT=j['xT'], start=j['start'], u=j['u'], Y=j['Y']) for j in jobs], t, blob, 1, Hc, Kc, m)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        mid_bwd([dict(xT=j['xT'], start=j['start'], Y=j['Y'], ubar=j['ubar'], gx=j['gx'], gs=j['gs'], gslab=j['gslab'])
                 for j in jobs], t, blob, 1, Hc, Kc, m, want_x=True, want_params=True, x_cot_ones=True)
        torch.cuda.synchronize()
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    for st in steppers:
        dopri(st)
    midpoint()                                                      # (warm-up: code objects, allocator)
    rows = {st: [] for st in steppers}
    for _ in range(a.reps):                                         # (both: alternately, so that drift hits the two alike)
        for st in steppers:
            rows[st].append(dopri(st))
    mids = [midpoint() for _ in range(a.reps)]
    med = lambda v: sorted(v)[len(v) // 2]                          # noqa: E731
    mf, ms = med([r[0] for r in mids]), med([r[1] for r in mids])
    res = dict(shape=dict(d=d, H=H, K=K, m=m, paths_per_job=N, jobs=2, N_t=L))
    for st in steppers:
        # (the keys of the default invocation are those this tool has always printed; the tiled implementation's carry its name)
        pre = 'dopri5_' if st == 'vector' else 'dopri5_tiled_'
        recs = rows[st][-1][0]
        fwd, swp, tot = [r[1] for r in rows[st]], [r[2] for r in rows[st]], [r[1] + r[2] for r in rows[st]]
        if st == 'vector':
            res.update(attempts=[r.n_att for r in recs], accepted=[r.n_acc for r in recs])
        else:
            res.update(tiled_attempts=[r.n_att for r in recs], tiled_accepted=[r.n_acc for r in recs])
        res.update({pre + 'forward_ms': round(med(fwd), 3), pre + 'sweep_ms': round(med(swp), 3),
                    pre + 'total_ms': round(med(fwd) + med(swp), 3), pre + 'per_s': round(1e3 / (med(fwd) + med(swp)), 3)})
        if a.stepper != 'vector':
            res.update({pre + 'forward_min_max_ms': [round(min(fwd), 3), round(max(fwd), 3)],
                        pre + 'sweep_min_max_ms': [round(min(swp), 3), round(max(swp), 3)],
                        pre + 'total_min_max_ms': [round(min(tot), 3), round(max(tot), 3)]})
    res.update(midpoint_forward_ms=round(mf, 3), midpoint_sweep_ms=round(ms, 3), midpoint_total_ms=round(mf + ms, 3),
               midpoint_per_s=round(1e3 / (mf + ms), 3), reps=a.reps, statistic='median')
    if a.stepper != 'vector':
        res.update(stepper=a.stepper, midpoint_family=net.family)
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
