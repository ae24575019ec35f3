"""solver 'dopri5' at the headline shape: what one u_theta forward + sweep costs with the adaptive stepper against midpoint.

Shape: cube, d = 20, two groups of 4096 paths (the interior sample u is integrated on and the boundary sample) sharing one
sorted N_t = 32 grid, the YAML network (u_hidden_dim 20, u_hidden_hidden_dim 10, u_layers 8), Xavier weights with zero biases as
at initialisation.  The dopri5 forward is one launch pair (init) plus chunks of attempt launches for both jobs, the sweep one
launch with parameter and x gradients (the generator's fused form) -- the stepper part of a dopri5 generator sub-step, measured
through kernels.dopri5_fwd / dopri5_sweep.

    python tools/dopri5_rate.py [--reps 5] [--out profiles/dopri5_rate.json]
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
    a = ap.parse_args()
    d, H, K, m, N, L = 20, 20, 10, 8, 4096, 32
    torch.manual_seed(0)
    net = nets.XNODE(H, 1, None, None, {'dim': d}, K, m, None, solver='dopri5')
    blob = net.bind(torch.device('cuda')).data
    Hc, Kc = net.kdims
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

    def dopri():
        t0 = time.perf_counter()
        recs = KN.dopri5_fwd(fwd_jobs, t, blob, Hc, Kc, m, H)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        KN.dopri5_sweep([dict(j, rec=r) for j, r in zip(jobs, recs)], t, blob, Hc, Kc, m, want_x=True, want_params=True,
                        x_cot_ones=True)
        torch.cuda.synchronize()
        return recs, (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    def midpoint():
        t0 = time.perf_counter()
        KN.ode_fwd_multi([dict(xT=j['xT'], start=j['start'], u=j['u'], Y=j['Y']) for j in jobs], t, blob, 1, Hc, Kc, m)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        KN.ode_bwd_multi([dict(xT=j['xT'], start=j['start'], Y=j['Y'], ubar=j['ubar'], gx=j['gx'], gs=j['gs'], gslab=j['gslab'])
                          for j in jobs], t, blob, 1, Hc, Kc, m, want_x=True, want_params=True, x_cot_ones=True)
        torch.cuda.synchronize()
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    dopri()
    midpoint()                                                      # (warm-up: code objects, allocator)
    rows = [dopri() for _ in range(a.reps)]
    mids = [midpoint() for _ in range(a.reps)]
    recs = rows[-1][0]
    fwd = sorted(r[1] for r in rows)[len(rows) // 2]
    swp = sorted(r[2] for r in rows)[len(rows) // 2]
    mf = sorted(r[0] for r in mids)[len(mids) // 2]
    ms = sorted(r[1] for r in mids)[len(mids) // 2]
    res = dict(shape=dict(d=d, H=H, K=K, m=m, paths_per_job=N, jobs=2, N_t=L),
               attempts=[r.n_att for r in recs], accepted=[r.n_acc for r in recs],
               dopri5_forward_ms=round(fwd, 3), dopri5_sweep_ms=round(swp, 3), dopri5_total_ms=round(fwd + swp, 3),
               dopri5_per_s=round(1e3 / (fwd + swp), 3),
               midpoint_forward_ms=round(mf, 3), midpoint_sweep_ms=round(ms, 3), midpoint_total_ms=round(mf + ms, 3),
               midpoint_per_s=round(1e3 / (mf + ms), 3), reps=a.reps, statistic='median')
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
