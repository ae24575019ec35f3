#!/usr/bin/env python3
"""bench.py -- WAN training-steps/sec on the BASELINE.json headline workload:
d=20 time-independent cube (Ex4_1 functions), N_r = N_b = 4096 paths, N_t = 32, YAML hyper-parameters, float64.

    python bench.py [--gpus N --steps K --warmup W --dump-outputs DIR]
N > 1: one rank per GPU.  Started under torch.distributed.run (WORLD_SIZE set) this process IS a rank; started plainly,
`python bench.py --gpus N` launches `python -m torch.distributed.run --nproc-per-node N bench.py <same arguments>` itself as
a child process (before anything touches the GPU), relays rank 0's JSON line and exits with the child's code -- the
reference's nn.DataParallel needs no launcher either (src/training.py:93-97).

A "step" is one optimiser sub-step of the adversarial loop (src/training.py:125-138 generator, :151-162 discriminator)
on synthetic sampled paths already resident in HBM; the timed region cycles generator, generator, discriminator
(n1 = 2, n2 = 1) and contains every kernel of the sub-step including the fused Adam update.  Resampling, diagnostics
and file I/O of the outer loop are outside the timed region (reported separately in `extras`).

Default scaling is WEAK: every rank holds its own N_r = 4096 interior + 4096 boundary paths (global batch 4096 x n_gpus),
the loss couples them through one (generator) or two (discriminator) small all-reduces per sub-step (dist.py); `value` =
sub-steps/s x n_gpus, i.e. 4096-path sub-steps per second over the whole job.
`--global-paths N` switches to STRONG scaling, the way BASELINE configs[2] / configs[3] are stated (a FIXED global batch
sharded over the GPUs, the reference's scatter along dim 0, src/training.py:93-97): every rank takes its contiguous
share of N interior + N boundary paths (dist.World.bounds) and `value` is the plain rate of global sub-steps.
ONE command answers both questions: without --global-paths the run also times two FIXED global batches after the headline
-- the headline batch itself (4096 global paths) and BASELINE configs[2] (d = 50, N_t = 64, 16384 global paths) -- sharded
over the same ranks, and reports them under `extras.strong` (steps_per_s of a fixed batch at --gpus 1, 2, 4, 8 is the
strong-scaling curve; `value` stays the weak product); `extras.rccl` records how many ranks the exchange saw and whether it
ran inside the captured sub-step graphs.

Timed region: exactly `--steps` sub-steps cycling g, g, d (the cycle runs on from the warm-up, which is padded so that the
first timed sub-step is a generator one), repeated `--repeats` times back to back (default once), each repeat bracketed by
barrier + synchronize; the reported figure is the MEDIAN repeat (`ms_per_step` x `steps` = that repeat's wall time; all
repeats are listed in extras.repeat_ms).

`--dump-outputs DIR`: after the timed regions, rank 0 writes what the timed path left its caller after its last sub-step,
float64, as DIR/<name>.npy: `theta` and `phi` (the updated parameters of u_theta and of the test network), `loss_u`
and `loss_v` (Engine.loss_u() / loss_v()), `grad_u` and `grad_v` (the gradients the last generator / discriminator Adam
update applied).  The inputs are seeded, so two builds run with the same arguments can be compared array by array.

Prints ONE JSON line (rank 0).  Extra objects: `roofline` for the dominant kernel (HIP-event timed on the launch
stream), `cpu_baseline` (the oracle = CPU restatement of the reference, timed on this host, N=1 only).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP64_MATRIX_TFLOPS = 78.6   # MI355X dense FP64 matrix peak (spec); v_mfma_f64_16x16x4 measured 77.6 (profiles/r01_probe_fp64.txt)


def workload_params(d, n_r, n_b, n_t):
    return {'alpha': 100000000, 'u_layers': 8, 'u_hidden_dim': 20, 'u_hidden_hidden_dim': 10, 'v_layers': 9,
            'v_hidden_dim': 50, 'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False,
            'solver': 'midpoint', 'dim': d, 'N_t': n_t, 'N_r': n_r, 'N_b': n_b, 'T0': 0, 'T': 1, 'shape_param': [-1, 1],
            'iterations': 1, 'domain': 'Hypercube'}


def algorithmic_macs(p):
    """per-unit multiply-accumulates of the two nets."""
    d, H, K, m, W, q, L = p['dim'], p['u_hidden_dim'], p['u_hidden_hidden_dim'], p['u_layers'], p['v_hidden_dim'], p['v_layers'], p['N_t']
    macs_F = (d + 1 + H) * K + (m - 1) * K * K + K * H
    path_u = 2 * (L - 1) * macs_F + (H + 2 * H * H) + L * H
    macs_v = (d + 1) * W + q * W * W + W
    return macs_F, path_u, macs_v


def self_launch(argv, gpus):
    """`python bench.py --gpus N` without a launcher: start the N ranks as a CHILD process (never exec: this process may not
    be replaced once a GPU runtime is up, and here nothing has touched it yet), pass the output through, return its code."""
    import socket
    import subprocess
    with socket.socket() as so:                     # a free rendezvous port on the loop-back interface
        so.bind(('127.0.0.1', 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.setdefault('MASTER_ADDR', '127.0.0.1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(gpus), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=6)
    ap.add_argument('--dim', type=int, default=20)
    ap.add_argument('--n_r', type=int, default=4096)
    ap.add_argument('--n_b', type=int, default=4096)
    ap.add_argument('--n_t', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=1, help='timed regions of --steps sub-steps each; the median is reported')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None, help='after the timed steps, write what the timed path '
                    'computed in its last sub-step as DIR/<name>.npy (float64)')
    ap.add_argument('--global-paths', type=int, default=0, help='strong scaling: a fixed global batch of this many interior '
                    '(and boundary) paths, sharded over the ranks (configs[2]: --dim 50 --n_t 64 --global-paths 16384; '
                    'configs[3]: --dim 100 --global-paths 65536)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--train-iters', type=int, default=600, help='outer iterations of real training (with resampling) for '
                    'the rel-L2 figure, outside the timed region; 0 disables')
    ap.add_argument('--no-strong', action='store_true', help='N > 1 without --global-paths: skip the two strong-scaling workloads '
                    'that are timed after the weak-scaling headline (extras.strong)')
    ap.add_argument('--no-solo', action='store_true', help='skip the extra full-grid launches of the dominant kernel '
                    '(roofline.solo_full_grid), so that a profiler run only sees production launches')
    args = ap.parse_args()
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(self_launch(sys.argv[1:], args.gpus))

    import configs.Ex4_1_funcs as P
    from xnode_wan_pde_solver_amd import dist as xdist, kernels as KN
    from src.training import NODE_WAN_solver
    from src.dataset import Comb_loader
    from utils.auxillary_funcs import rel_err

    world, local = xdist.init_from_env()
    size = world.size if world is not None else 1
    rank = world.rank if world is not None else 0
    if size > 1:
        # N > 1: a rank stuck in a collective (an exchange inside a captured sub-step that never completes, a peer that died without
        # its exception reaching the launcher) would hang the job until the driver's own clock ends it without a word.  A watchdog
        # thread ends THIS process loudly instead; the launcher then stops the others and returns non-zero.  (A healthy run of every
        # workload of this file takes 1 - 2 minutes per rank.)  XW_BENCH_WATCHDOG_S: seconds, 0 disables.
        import threading
        limit = float(os.environ.get('XW_BENCH_WATCHDOG_S', '900'))

        def _stuck():
            sys.stderr.write('bench.py: rank %d of %d made no end within %.0f s -- a collective that never completed? '
                             '(XW_CAPTURE_EXCHANGE=0 keeps the exchanges out of the captured sub-steps, XW_NATIVE_ALLREDUCE=0 '
                             'routes them through torch.distributed)\n' % (rank, size, limit))
            sys.stderr.flush()
            os._exit(4)
        if limit > 0:
            wd = threading.Timer(limit, _stuck)
            wd.daemon = True
            wd.start()
    if size != args.gpus:
        raise SystemExit('--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run --nproc-per-node %d' % (args.gpus, size, args.gpus))
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    strong = args.global_paths > 0
    if strong:                                            # this rank's contiguous share of the fixed global batch
        base, rem = divmod(args.global_paths, size)
        args.n_r = args.n_b = base + (1 if rank < rem else 0)
    params = workload_params(args.dim, args.n_r, args.n_b, args.n_t)
    n_glob = args.global_paths if strong else args.n_r * size
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit('--steps must be >= 1 and --warmup >= 0')

    torch.manual_seed(0)                                  # identical initial parameters and time grid on every rank
    S = NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, dev, './',
                        func_u_sol=P.func_u_sol, p=2, world=world)
    eng, s = S.engine, S.setup
    domain = S.domain(s['shape_param'], s['dim'], s['T0'], s['T'], s['N_t'])
    torch.manual_seed(1000 + rank)                        # every rank draws its own shard of the global Monte-Carlo batch
    t_s0 = time.time()
    pts = Comb_loader(s['N_r'], s['N_b'], domain, dev)
    du, dv, bd = pts[0]
    G = eng.load_group(du, dv, bd, domain, n_glob=n_glob, nb_glob=n_glob if strong else s['N_b'] * size)
    torch.cuda.synchronize()
    t_sample = time.time() - t_s0

    schedule = ['g', 'g', 'd']

    def barrier():
        if world is not None:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    def timed_regions(eng_, G_, steps, warmup, repeats):
        """`repeats` timed regions of exactly `steps` sub-steps of group G_ (the g, g, d cycle running on across them), each
        bracketed by barrier + synchronize, every one as long as its slowest rank; returns (seconds per region, untimed extra
        warm-up sub-steps)"""
        pos = [0]                                         # sub-steps run so far: position in the g, g, d cycle

        def run_(n):
            for _ in range(n):
                if schedule[pos[0] % 3] == 'g':
                    eng_.generator_step(G_)
                else:
                    eng_.discriminator_step(G_)
                pos[0] += 1
        run_(warmup)
        # The shader clock needs ~30 ms of load to settle (repeats of a 3 ms region: 3.48, 3.44, 3.32, 3.25, 3.20 ms): when the
        # requested warm-up is shorter than 54 sub-steps, untimed sub-steps are added up to that, and up to a whole cycle so that
        # the first timed sub-step is a generator one (extras.extra_warmup_steps)
        # (a fixed count, not a timed loop: every rank must run the same number of sub-steps -- they contain collectives)
        extra = max(0, 54 - warmup)
        extra += -(warmup + extra) % 3
        run_(extra)
        region_ = []
        for _ in range(max(repeats, 1)):
            barrier()
            t0 = time.perf_counter()
            run_(steps)
            torch.cuda.synchronize()
            barrier()
            region_.append(time.perf_counter() - t0)
        if world is not None:                                 # a region is as long as its slowest rank
            on_host = torch.distributed.get_backend() == 'gloo'
            te = torch.tensor(region_, dtype=torch.float64, device='cpu' if on_host else dev)
            torch.distributed.all_reduce(te, op=torch.distributed.ReduceOp.MAX)
            region_ = [float(x) for x in te.tolist()]
        return region_, extra

    def run(n, offset=0):
        for i in range(n):
            if schedule[(offset + i) % 3] == 'g':
                eng.generator_step(G)
            else:
                eng.discriminator_step(G)

    region, extra_warmup = timed_regions(eng, G, args.steps, args.warmup, args.repeats)
    elapsed = sorted(region)[len(region) // 2]            # median repeat
    if args.dump_outputs and rank == 0:
        # what the timed path handed its caller after its last sub-step (before anything below steps the engine again)
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        dump = {'theta': eng.theta.data, 'phi': eng.phi.data, 'loss_u': eng.loss_u().reshape(1), 'loss_v': eng.loss_v().reshape(1),
                'grad_u': eng.grad_u, 'grad_v': eng.grad_v}
        for name, t in dump.items():
            np.save(os.path.join(args.dump_outputs, name + '.npy'), t.detach().to('cpu', torch.float64).numpy())
    steps_per_s = args.steps / elapsed
    finite = bool(torch.isfinite(eng.scal[4]).item() and torch.isfinite(eng.theta.data).all().item())

    # ---- per-kernel timing with events on the launch stream (instrumented pass, outside the timed region) ------------
    names = ['disc_fwd', 'disc_gradx', 'ode_fwd_multi', 'ode_bwd_multi', 'weak_partials', 'bdry_partials', 'gen_cotangents',
             'disc_cotangent', 'disc_bwd', 'adam', 'slab_sum', 'losses']

    def kernel_pass(eng_, G_, params_, n_paths, nb_paths):
        """every kernel launch of 9 sub-steps (3 cycles) bracketed by an event pair on the launch stream, serial and eager;
        returns (per-kernel times, algorithmic FLOP per launch, the dominant kernel, its achieved TFLOP/s)"""
        graphs_, streams_ = eng_.use_graphs, eng_.use_streams
        eng_.use_graphs = eng_.use_streams = False             # serial, eager: one event pair per kernel launch
        records, originals = {}, {}

        def wrap(name, fn):
            def inner(*a, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = fn(*a, **kw)
                e1.record()
                key = name
                if name == 'ode_bwd_multi':
                    key = ('ode_bwd_params' if kw.get('want_params') else 'ode_bwd_x') + '_%djob' % len(a[0])
                if name == 'ode_fwd_multi':
                    key = 'ode_fwd_%djob' % len(a[0])
                records.setdefault(key, []).append((e0, e1))
                return r
            return inner
        for n_ in names:
            originals[n_] = getattr(KN, n_)
            setattr(KN, n_, wrap(n_, originals[n_]))
        prof_steps = 9
        try:
            for i in range(prof_steps):
                if schedule[i % 3] == 'g':
                    eng_.generator_step(G_)
                else:
                    eng_.discriminator_step(G_)
            torch.cuda.synchronize()
        finally:
            for n_ in names:
                setattr(KN, n_, originals[n_])
            eng_.use_graphs, eng_.use_streams = graphs_, streams_
        kern_ = {k: {'launches_per_step': len(v) / prof_steps, 'avg_ms': sum(a.elapsed_time(b) for a, b in v) / len(v)}
                 for k, v in records.items()}
        for k in kern_:
            kern_[k]['ms_per_step'] = kern_[k]['avg_ms'] * kern_[k]['launches_per_step']
        _, path_u_, macs_v_ = algorithmic_macs(params_)
        Pn_ = n_paths * params_['N_t']
        flops_ = {                                             # algorithmic FLOP (2 x MAC) per launch, SURVEY section 8(d)
            # value + d/dt tangent at all points, reverse pass at the N points of t_0; with the input layer's spatial columns applied
            # once per path (engine: from d = XW_XPROJ_MIN_D on) the d W multiply-adds per point it no longer does are not counted
            'disc_fwd': 2.0 * ((2 * Pn_ + n_paths) * macs_v_ - ((Pn_ - n_paths) * params_['dim'] * params_['v_hidden_dim']
                                                                if G_.ptr('xproj') else 0)),
            'disc_bwd': 2.0 * 2 * Pn_ * macs_v_,               # reverse chain + weight-gradient contraction (recompute not counted)
            'ode_fwd_1job': 2.0 * n_paths * path_u_,
            'ode_fwd_2job': 2.0 * (n_paths + nb_paths) * path_u_,
            'ode_bwd_x_1job': 2.0 * n_paths * path_u_,         # adjoint chain (recompute not counted)
            'ode_bwd_params_1job': 2.0 * 2 * n_paths * path_u_,   # adjoint chain + weight-gradient contraction
            'ode_bwd_params_2job': 2.0 * 2 * (n_paths + nb_paths) * path_u_,
            'ode_bwd_params_3job': 2.0 * 2 * (2 * n_paths + nb_paths) * path_u_,   # (compact schedule: sweeps A, boundary, B in one launch)
        }
        dom_ = max((k for k in kern_ if k in flops_), key=lambda k: kern_[k]['ms_per_step'])
        return kern_, flops_, dom_, flops_[dom_] / (kern_[dom_]['avg_ms'] * 1e-3) / 1e12

    graphs_on, streams_on = eng.use_graphs, eng.use_streams
    kern, alg_flops, dominant, ach = kernel_pass(eng, G, params, s['N_r'], s['N_b'])
    macs_F, path_u, macs_v = algorithmic_macs(params)
    Pn, N, Nb = s['N_r'] * s['N_t'], s['N_r'], s['N_b']
    # HBM bytes per launch: NOT measurable inside this process (rocprofv3 --pmc passes, separate runs); taken from the
    # newest committed counter summary and labelled as such (roofline.traffic_source); null when there is none for the workload
    traffic, traffic_by_variant, traffic_source = None, None, None
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc_traffic.json')))
    pmc_path = cands[-1] if cands else ''
    default_workload = (args.dim, args.n_r, args.n_b, args.n_t) == (20, 4096, 4096, 32)
    if os.path.exists(pmc_path) and default_workload:
        pmc = json.load(open(pmc_path))['kernels']
        # k_disc_fwd runs in two variants: plain (generator sub-steps, 3.9 MB of inputs + outputs) and with the activation
        # record for the backward (discriminator sub-step, +524 MB of stores by design): average over the g,g,d cycle, like avg_ms
        # (kernel names as rocprofv3 prints them, matched by prefix: k_disc_fwd<W, record?, ticket queue?>)
        prefixes = {'disc_fwd': ['k_disc_fwd<50,false', 'k_disc_fwd<50,true'],
                    'disc_bwd': ['k_disc_rec<50,9,1']}.get(dominant, [])
        keys = [next((k for k in sorted(pmc) if k.startswith(pre)), None) for pre in prefixes]
        if keys and all(k is not None for k in keys):
            wts = [schedule.count('g'), schedule.count('d')] if len(keys) == 2 else [1]     # launches per g,g,d cycle
            traffic = int(sum(w_ * pmc[k]['hbm_bytes_per_launch_corrected'] for w_, k in zip(wts, keys)) / sum(wts))
            traffic_by_variant = {k: pmc[k]['hbm_bytes_per_launch_corrected'] for k in keys}
            traffic_source = 'profiles/' + os.path.basename(pmc_path) + ' (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, not this run)'
    roofline = {'bound': 'mfma', 'kernel': dominant, 'achieved': round(ach, 3), 'peak': PEAK_FP64_MATRIX_TFLOPS,
                'unit': 'TFLOP/s', 'frac': round(ach / PEAK_FP64_MATRIX_TFLOPS, 4), 'traffic': traffic,
                'alg_flop_per_launch': alg_flops[dominant], 'avg_launch_ms': round(kern[dominant]['avg_ms'], 4)}
    if traffic_by_variant:
        roofline['traffic_by_variant'] = traffic_by_variant
        roofline['traffic_source'] = traffic_source
    if dominant == 'disc_fwd' and not args.no_solo:
        # The production launches above are capped below the resident block
        # slots (Engine.v_blocks, v_blocks_disc) so that the stepper's waves find room next to them; the same kernel given the
        # whole chip, for reference:
        roofline['launch_blocks'] = {'generator_substep': eng.v_blocks, 'discriminator_substep': eng.v_blocks_disc, 'slots': 512}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        full = lambda: KN.disc_fwd(G.xvT, G.t, eng.phi.data, eng.W, eng.q, v=G.v, vt=G.vt, gxv=G.gxv, gtv=G.gtv,   # noqa: E731
                                   ngrad=G.N, max_blocks=0, xproj=G.xproj if G.ptr('xproj') else None)
        if G.ptr('xproj'):
            KN.disc_xproj(G.xvT, eng.phi.data, eng.W, out=G.xproj)
        for _ in range(3):
            full()
        ev[0].record()
        for _ in range(10):
            full()
        ev[1].record()
        torch.cuda.synchronize()
        ms_full = ev[0].elapsed_time(ev[1]) / 10
        roofline['solo_full_grid'] = {'avg_launch_ms': round(ms_full, 4),
                                      'achieved': round(alg_flops[dominant] / (ms_full * 1e-3) / 1e12, 3),
                                      'frac': round(alg_flops[dominant] / (ms_full * 1e-3) / 1e12 / PEAK_FP64_MATRIX_TFLOPS, 4)}
    # (large d: the input layer's spatial columns are applied once per path, not once per point -- multiply-adds not done are not counted)
    hoisted = (Pn - N) * params['dim'] * params['v_hidden_dim'] if G.ptr('xproj') else 0
    gen_flops = 2.0 * (2 * Pn * macs_v - hoisted + 4 * N * path_u + 3 * Nb * path_u)
    dis_flops = 2.0 * (3 * Pn * macs_v - hoisted + 2 * N * path_u)
    step_flops = (2 * gen_flops + dis_flops) / 3.0
    # SURVEY 8(d) asks for both fractions of the whole sub-step: FP64 (the binding one) and HBM (the reference layout's
    # bytes X, XV, BX [*, L, d+1] f32 + ~48 B/point of [N, L] f64 side streams -- a few per cent at most by construction)
    d_ = s['dim']
    bytes_step = 4.0 * (d_ + 1) * (2 * Pn + Nb * s['N_t']) + 48.0 * Pn
    per_gpu_rate = steps_per_s                             # every rank steps through its own shard (sizes above are the shard's)
    whole = {'alg_gflop_per_step_avg': round(step_flops / 1e9, 2),
             'achieved_tflops': round(step_flops * per_gpu_rate / 1e12, 3),
             'frac_fp64_matrix_peak': round(step_flops * per_gpu_rate / 1e12 / PEAK_FP64_MATRIX_TFLOPS, 4),
             'ref_layout_mbytes_per_step': round(bytes_step / 1e6, 1),
             'frac_hbm_peak': round(bytes_step * per_gpu_rate / 8.0e12, 5)}
    # ... and what the memory system actually moves: HBM bytes per sub-step from the committed counter passes (the activation
    # store of the stepper and the test network's record are deliberate store-instead-of-recompute trades: ~30 x the reference
    # layout's bytes).  Preferred source: the `cycle` section of the counter summary (all kernels of whole g,g,d cycles,
    # tools/cycle_only.py under rocprofv3 --pmc); otherwise the per-kernel averages x this run's launches per sub-step.
    if os.path.exists(pmc_path) and default_workload:
        pmc_all = json.load(open(pmc_path))
        counter_bytes, how = None, None
        if isinstance(pmc_all.get('cycle'), dict) and pmc_all['cycle'].get('hbm_bytes_per_substep_corrected'):
            counter_bytes = float(pmc_all['cycle']['hbm_bytes_per_substep_corrected'])
            how = 'cycle section: every kernel of %s g,g,d cycles' % pmc_all['cycle'].get('cycles', '?')
        else:
            pk = pmc_all['kernels']
            first = lambda pre: next((pk[k]['hbm_bytes_per_launch_corrected'] for k in sorted(pk) if k.startswith(pre)), None)  # noqa: E731
            n_g, n_d = schedule.count('g'), schedule.count('d')
            per_launch = {'disc_bwd': first('k_disc_rec<'), 'ode_fwd_2job': first('k_ode_fwd<20,10,8,1,1>'), 'ode_fwd_1job': first('k_ode_fwd<20,10,8,1,2>'),
                          'ode_bwd_x_1job': first('k_ode_bwd<'), 'ode_bwd_params_1job': first('k_ode_bwd_duo<'), 'ode_bwd_params_2job': first('k_ode_bwd_duo<'),
                          'ode_bwd_params_3job': first('k_ode_bwd_duo<'), 'weak_partials': first('k_weak_partials'), 'adam': first('k_adam'),
                          'slab_sum': first('k_slab_sum'), 'disc_cotangent': first('k_disc_cot')}
            fg, fd = first('k_disc_fwd<50,false'), first('k_disc_fwd<50,true')
            if fg is not None and fd is not None:
                per_launch['disc_fwd'] = (n_g * fg + n_d * fd) / (n_g + n_d)
            if all(per_launch.get(k) is not None for k in kern if k in per_launch) and 'disc_fwd' in per_launch:
                counter_bytes = sum(per_launch[k] * v['launches_per_step'] for k, v in kern.items() if k in per_launch)
                how = 'per-kernel averages x launches per sub-step of this run'
        if counter_bytes:
            whole['counter_mbytes_per_step'] = round(counter_bytes / 1e6, 1)
            whole['frac_hbm_peak_counter'] = round(counter_bytes * per_gpu_rate / 8.0e12, 4)
            whole['counter_source'] = 'profiles/' + os.path.basename(pmc_path) + ' (' + how + '; counter passes of another run of this command)'
            roofline['traffic_ratio'] = round(counter_bytes / bytes_step, 1)      # HBM bytes moved / algorithmic bytes of the reference layout, per sub-step

    # ---- opt-in exact optimisation, reported separately: reuse v, dv/dt, nabla_x v(t_0) while phi is unchanged ----------
    if world is None:
        eng.reuse_test_net = True
        run(6)
        torch.cuda.synchronize()
        r0 = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize()
        reuse_rate = args.steps / (time.perf_counter() - r0)
        eng.reuse_test_net = False
    else:
        reuse_rate = None

    # ---- real training (resampling every outer iteration) for the rel-L2 figure ----------------------------------------
    extras = {'sample_and_tabulate_s': round(t_sample, 4), 'finite': finite, 'structure': eng.structure.describe(),
              'extra_warmup_steps': extra_warmup, 'hip_graphs': graphs_on, 'side_streams': streams_on,
              'steps_per_s_with_test_net_reuse_optin': None if reuse_rate is None else round(reuse_rate, 1),
              'serial_kernel_ms_per_step': round(sum(v['ms_per_step'] for v in kern.values()), 4),
              'repeat_ms': [round(1e3 * x, 3) for x in region], 'reported_repeat': 'median',
              'exchange': None if world is None else ('xw_allreduce (RCCL), captured in the sub-step graphs' if eng.capture_exchange
                                                      else 'torch.distributed between graph segments')}
    if world is not None:
        # RCCL as the job sees it: one sum of ones through the library's own entry point (the exchange of the sub-steps), and
        # whether that exchange sits inside the captured sub-step graphs
        ones = torch.ones(1, dtype=torch.float64, device=dev)
        world.all_reduce(ones)
        extras['rccl'] = {'ranks_seen': int(round(float(ones[0]))), 'native_communicator': world.comm is not None,
                          'in_graph': bool(eng.capture_exchange and any(k.startswith('gen_dist') for k in G.graphs)
                                           and any(k.startswith('disc_dist') for k in G.graphs)),
                          'backend': torch.distributed.get_backend()}
    if not strong and not args.no_strong:
        # ---- the same command also answers the STRONG-scaling question (a FIXED global batch over the ranks, the way
        # BASELINE configs[2] / configs[3] are stated and the way the reference's nn.DataParallel scatters, src/training.py:93-97):
        # the headline batch (4096 global paths) and configs[2] (d = 50, N_t = 64, 16384 global paths), each as its own solver
        # on this rank's contiguous share; `value` above stays the weak product.  Compare extras.strong[*].steps_per_s of runs
        # with different --gpus (and profiles/r04_other_configs_1gpu.md for one GPU) for the 1 -> 8 speed-up of a fixed batch.
        def strong_workload(dim, n_t, gpaths, tag, steps=30, warmup=6, repeats=3):
            base_, rem_ = divmod(gpaths, size)
            n_loc = base_ + (1 if rank < rem_ else 0)
            p_ = workload_params(dim, n_loc, n_loc, n_t)
            torch.manual_seed(0)
            S_ = NODE_WAN_solver(p_, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, dev, './', func_u_sol=P.func_u_sol,
                                 p=2, world=world)
            e_, s_ = S_.engine, S_.setup
            dom_ = S_.domain(s_['shape_param'], s_['dim'], s_['T0'], s_['T'], s_['N_t'])
            torch.manual_seed(1000 + rank)
            du_, dv_, bd_ = Comb_loader(n_loc, n_loc, dom_, dev)[0]
            G_ = e_.load_group(du_, dv_, bd_, dom_, n_glob=gpaths, nb_glob=gpaths)
            reg_, _ = timed_regions(e_, G_, steps, warmup, repeats)
            el_ = sorted(reg_)[len(reg_) // 2]
            k_, f_, d_k, a_ = kernel_pass(e_, G_, p_, n_loc, n_loc)
            fused_x = e_.pollution == 1.0 and not e_.adjoint
            out_ = {'workload': tag, 'scaling': 'strong', 'global_paths': gpaths, 'paths_per_rank': [base_, base_ + (1 if rem_ else 0)],
                    'steps': steps, 'repeats': repeats, 'steps_per_s': round(steps / el_, 2), 'ms_per_step': round(1e3 * el_ / steps, 4),
                    'finite': bool(torch.isfinite(e_.scal[4]).item() and torch.isfinite(e_.theta.data).all().item()),
                    'exchange': None if world is None else ('xw_allreduce (RCCL), captured in the sub-step graphs' if e_.capture_exchange else 'torch.distributed between graph segments'),
                    'schedule_rank0': {'generator': 'compact' if e_._compact(G_, fused_x, bool(G_.Nb and G_.same_grid)) else 'wide',
                                       'narrow_tiles_forward': bool(e_._narrow_ok([e_._job(G_, 'i'), e_._job(G_, 'b')], alone=False, forward=True))},
                    'roofline_rank0': {'bound': 'mfma', 'kernel': d_k, 'achieved': round(a_, 3), 'peak': PEAK_FP64_MATRIX_TFLOPS, 'unit': 'TFLOP/s',
                                       'frac': round(a_ / PEAK_FP64_MATRIX_TFLOPS, 4), 'avg_launch_ms': round(k_[d_k]['avg_ms'], 4),
                                       'alg_flop_per_launch': f_[d_k]}}
            del S_, G_
            torch.cuda.empty_cache()
            return out_
        try:
            if world is not None and os.environ.get('XW_BENCH_FAIL_RANK') == str(rank):       # (test hook: a rank that dies mid-way)
                raise RuntimeError('XW_BENCH_FAIL_RANK=%d' % rank)
            extras['strong'] = [strong_workload(20, 32, 4096, 'headline batch: Ex4_1 cube d=20, 4096 global paths, N_t=32 (configs[1] sharded)'),
                                strong_workload(50, 64, 16384, 'configs[2]: Ex4_1 cube d=50, 16384 global paths, N_t=64')]
        except Exception as e:
            if world is None:         # one process: never at the expense of the headline line
                extras['strong'] = {'error': repr(e)[:300]}
            else:
                # Several ranks: the others are inside (or on their way into) a collective of these workloads.  Catching the
                # exception here and walking on would leave them waiting for ever -- a rank that fails ENDS THE JOB: the launcher
                # (torch.distributed.run) sees the dead worker, stops the remaining ranks and returns non-zero.
                import traceback
                sys.stderr.write('bench.py: rank %d failed in the strong-scaling workloads, ending the job:\n' % rank)
                traceback.print_exc()
                sys.stderr.flush()
                os._exit(3)
        if world is not None:
            # ... and a rank whose workloads ran but produced garbage says so to all of them (one MIN all-reduce: every rank
            # prints / returns the same verdict)
            ok = torch.tensor([1.0 if all(w_['finite'] for w_ in extras['strong']) else 0.0], dtype=torch.float64,
                              device='cpu' if torch.distributed.get_backend() == 'gloo' else dev)
            torch.distributed.all_reduce(ok, op=torch.distributed.ReduceOp.MIN)
            extras['strong_finite_on_every_rank'] = bool(ok[0] == 1.0)
    if args.train_iters > 0 and world is None:
        # The reference's own acceptance rule is a stopping rule: train until the relative L2 error drops below 0.01
        # (configs/Ex4_1_funcs.py:36-37).  Same rule here, on the fixed held-out sample (16,384 paths, seed 12345), checked
        # every 25 outer iterations, at most --train-iters of them; adversarial training oscillates, so the value at an
        # arbitrary iteration count is not "the" error -- the trajectory is listed.
        torch.manual_seed(0)
        S2 = NODE_WAN_solver(dict(params, iterations=25), P.func_a, P.func_b, P.func_c, P.func_h, P.func_f,
                             P.func_g, dev, './', func_u_sol=P.func_u_sol, p=2)
        rng = torch.get_rng_state()
        torch.manual_seed(12345)
        hold = S2.domain(s['shape_param'], s['dim'], s['T0'], s['T'], s['N_t'])
        Xh = hold.interior(16384)
        torch.set_rng_state(rng)
        cwd = os.getcwd()
        import shutil
        import tempfile
        work = tempfile.mkdtemp(prefix='xnwan_bench_')     # train() writes its JSON logs and weights into the working directory
        os.chdir(work)
        traj, wall, done, calls = [], 0.0, 0, []
        try:
            while done < args.train_iters:
                tt0 = time.time()
                S2.train(report=False)
                torch.cuda.synchronize()
                calls.append(time.time() - tt0)
                wall += calls[-1]
                done += 25
                rng = torch.get_rng_state()
                traj.append(round(float(rel_err(Xh, S2.u_net, P.func_u_sol, 2, hold.V(), 16384)), 5))
                torch.set_rng_state(rng)
                if traj[-1] < 0.01:
                    break
            # ... and one long call (no held-out evaluation in between): what an outer iteration costs once the loop's pipeline is full
            S2.iterations = 200
            torch.cuda.synchronize()
            tt0 = time.time()
            S2.train(report=False)
            torch.cuda.synchronize()
            steady = 1e3 * (time.time() - tt0) / 200
            # ... and the loop the reference's own CLI selects (main.py:51 passes the configs' acceptance rule as `stop`): the
            # hook is evaluated after every generator sub-iteration (and never taken here), every sub-iteration is synchronised
            S2.stop = lambda solver, pts, dom: P.stop(solver, pts, dom) and False
            S2.iterations = 100
            S2.train(report=False)
            torch.cuda.synchronize()
            tt0 = time.time()
            S2.train(report=False)
            torch.cuda.synchronize()
            hooked = 1e3 * (time.time() - tt0) / 100
            S2.stop = None
        finally:
            os.chdir(cwd)
        extras['train'] = {'outer_iterations': done, 'ms_per_outer_iteration_one_call_of_200': round(steady, 2),
                           'ms_per_outer_iteration_with_the_reference_stop_hook': round(hooked, 2), 'stopped_by': 'rel-L2 < 0.01 (reference stopping rule)' if traj[-1] < 0.01 else 'iteration cap',
                           'wall_s': round(wall, 2), 'ms_per_outer_iteration_incl_resampling_diagnostics_io': round(1e3 * wall / done, 2),
                           # (the first 25-iteration call carries the library load and the graph captures)
                           'ms_per_outer_iteration_after_the_first_call': round(1e3 * sum(calls[1:]) / (25 * len(calls[1:])), 2) if len(calls) > 1 else None,
                           'rel_l2_heldout_16384': traj[-1], 'rel_l2_heldout_every_25_iterations': traj}

        # BASELINE configs[4] (time-varying balls, Ex4_3, d = 10, N_r = N_b = 8192, N_t = 20) through the same train(): 11-20 groups
        # per sample, ~60 dependent sub-steps of ~400 paths per outer iteration -- host-bound by construction; reported
        # beside the headline, never part of `value`
        try:
            import numpy as np
            import configs.Ex4_3_funcs as P3
            c5 = {}
            os.chdir(work)
            for name in ('NSphere_TCone', 'NSphere_THourglass'):
                p5 = dict(params, dim=10, N_t=20, N_r=8192, N_b=8192, T0=0, T=1, shape_param=1.0, alpha=1e4, domain=name, iterations=3)
                torch.manual_seed(0)
                np.random.seed(0)
                S5 = NODE_WAN_solver(p5, P3.func_a, P3.func_b, P3.func_c, P3.func_h, P3.func_f, P3.func_g, dev, './',
                                     func_u_sol=P3.func_u_sol, p=2)
                S5.train(report=False)
                S5.iterations = 30
                torch.cuda.synchronize()
                tt0 = time.time()
                S5.train(report=False)
                torch.cuda.synchronize()
                c5[name] = round(1e3 * (time.time() - tt0) / 30, 2)
                del S5
            extras['train_config5_ms_per_outer_iteration'] = c5
        except Exception as e:       # (never at the expense of the headline line)
            extras['train_config5_ms_per_outer_iteration'] = {'error': repr(e)[:200]}
        finally:
            os.chdir(cwd)
            shutil.rmtree(work, ignore_errors=True)

    # ---- CPU baseline: the oracle (port of the reference's CPU/PyTorch path), bounded sample ---------------------------
    cpu = None
    if rank == 0 and size == 1 and not args.no_cpu_baseline:
        from oracle import refspec as R
        funcs = dict(h=P.func_h, f=P.func_f, g=P.func_g, a=P.func_a, b=P.func_b, c=P.func_c)
        # all host threads: the port's small tensor operations thrash on a many-core host (42 s for the two sub-steps at full size on
        # 128 threads against 4 s on one), so this leg is bounded to a quarter of the paths and scaled; `value` comes from the
        # full-size one-thread run below unless this one is faster
        qn = max(s['N_r'] // 4, 1)
        torch.manual_seed(0)
        O = R.Solver(dict(params, N_r=qn, N_b=qn), funcs, u_sol=P.func_u_sol, p=2)
        O.new_sample()
        c0 = time.perf_counter()
        O.generator_step()
        O.discriminator_step()
        c_el = time.perf_counter() - c0
        cpu = {'value': round(2 / (c_el * s['N_r'] / qn), 5), 'unit': 'steps/s', 'cores': torch.get_num_threads(), 'kind': 'port',
               'sample': '1 generator + 1 discriminator sub-step on N_r = N_b = %d paths (%.1f s), scaled x%d to the workload' % (qn, c_el, s['N_r'] // qn)}
        # one thread, the same two sub-steps at the FULL workload size (measured, not extrapolated: ~4 s on the driver box's host)
        nthr = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            torch.manual_seed(0)
            O1 = R.Solver(params, funcs, u_sol=P.func_u_sol, p=2)
            O1.new_sample()
            c1 = time.perf_counter()
            O1.generator_step()
            O1.discriminator_step()
            c1_el = time.perf_counter() - c1
        finally:
            torch.set_num_threads(nthr)
        one = {'value': round(2 / c1_el, 5), 'unit': 'steps/s', 'cores': 1,
               'sample': '1 generator + 1 discriminator sub-step at the full workload size, one thread (%.1f s)' % c1_el}
        allthr = dict(cpu)
        # `value` is the BETTER of the two runs (the port's small tensor ops thrash on a many-core host: one thread is usually
        # faster than all of them); both are kept
        if one['value'] > cpu['value']:
            cpu = dict(one, kind='port')
        cpu['all_threads'], cpu['one_thread'] = allthr, one
        # the port against the reference itself, both timed on the build container's host (8-core Xeon 2.1 GHz): BASELINE.md
        # section 2 has the reference at 0.075 sub-steps/s on this workload; tools/calibrate_oracle.py has the port there
        cal_path = os.path.join(ROOT, 'profiles', 'r02_oracle_calibration.json')
        if os.path.exists(cal_path) and default_workload:
            cpu['calibration'] = json.load(open(cal_path))

    if rank == 0:
        out = {
            'metric': ('WAN training-steps/sec (optimiser sub-steps, d=%d cube, %d global paths)' % (s['dim'], n_glob)) if strong
                      else 'WAN training-steps/sec (optimiser sub-steps, d=20 cube, N_r=4096 paths per GPU)',
            'value': round(steps_per_s * (1 if strong else size), 3), 'unit': 'steps/s', 'n_gpus': size, 'steps': args.steps,
            'warmup': args.warmup, 'repeats': max(args.repeats, 1),
            'ms_per_step': round(1e3 * elapsed / args.steps, 4), 'higher_is_better': True,
            'scaling': 'strong' if strong else 'weak', 'vs_baseline': None, 'dtype': 'f64', 'data': 'synthetic',
            'config': {'workload': ('Ex4_1 cube d=%d, %d global paths (interior and boundary) sharded over %d GPU(s), N_t=%d, midpoint, n1=2 n2=1'
                                    % (s['dim'], n_glob, size, s['N_t'])) if strong else
                                   ('Ex4_1 cube d=%d N_r=%d N_b=%d N_t=%d per GPU, midpoint, n1=2 n2=1 (configs[1])'
                                    % (s['dim'], s['N_r'], s['N_b'], s['N_t'])), 'global_paths': n_glob,
                       'parallelism': ('%d global paths sharded x%d (strong scaling: value = global sub-steps/s)' % (n_glob, size)) if strong else
                                      ('paths sharded x%d, %d paths per rank (weak scaling: value = sub-steps/s x ranks, i.e. %d-path '
                                       'sub-steps per second over the job; the global batch grows with the rank count; the same run '
                                       'times FIXED global batches too: extras.strong)' % (size, s['N_r'], s['N_r']))
                                      + '; 1 all-reduce per generator, 2 per discriminator sub-step'},
            # the two FIXED global batches timed over the same ranks (extras.strong has the details): at --gpus 1, 2, 4, 8 these
            # are the strong-scaling curves -- `value` above is the weak product (rate x ranks) and cannot answer that question
            'strong_headline_steps_per_s': (extras['strong'][0]['steps_per_s'] if isinstance(extras.get('strong'), list) else None),
            'strong_configs2_steps_per_s': (extras['strong'][1]['steps_per_s'] if isinstance(extras.get('strong'), list) else None),
            'roofline': roofline, 'cpu_baseline': cpu, 'whole_step': whole,
            'kernels': {k: {'ms': round(v['avg_ms'], 4), 'per_step': round(v['launches_per_step'], 2)} for k, v in sorted(kern.items())},
            'extras': extras,
        }
        print(json.dumps(out))
    if world is not None:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
