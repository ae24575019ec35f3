"""tools/stepper_digests.py OUT.json [forms] -- SHA-256 of what the fused stepper leaves behind, for comparing two libraries bit by bit
(profiles/r24_stepper_by_kernel.md): run it once per library (XW_LIBRARY) and per setting of the engine's switches (XW_MERGED_SWEEP,
XW_COMPACT_TILES, XW_GRAPHS), one fresh process each, and compare the JSON files on the host.
  forms     every form of tests/stepper_inventory.FORMS at (20,10,8), (32,12,3), (64,16,10) with euler, midpoint and rk4 (17 paths, 3
            times, d = 3, seeded, in a guarded arena: u, Y, the activation store, gx, gs, the slabs, whole tensors) and the duo sweep's
            spacer round
  always    three generator and two discriminator sub-steps (g, g, d, g, d) at six networks -- the three containers with midpoint, (64,16)
            with euler, (32,12) with rk4, (20,10) with the continuous adjoint --: theta, phi and the scalar block after each"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

out = {}


def put(name, t):
    t = t.detach().contiguous().cpu()
    out[name] = hashlib.sha256(t.numpy().tobytes()).hexdigest() + (' nonfinite' if t.is_floating_point() and not torch.isfinite(t).all() else '')


def forms():
    import guarded as G
    import stepper_inventory as SI
    from test_gpu_edges import DEVICE, _fused_oracle
    from xnode_wan_pde_solver_amd import kernels as KN
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    cases = [((H, K, m, method), 17, 3, 3, None) for H, K, m in ((20, 10, 8), (32, 12, 3), (64, 16, 10)) for method in SI.METHODS]
    cases.append(((20, 10, 8, 'midpoint'), 16 * (ncu + 1), 2, 3, ['fwd_store', 'duo']))          # the duo sweep's spacer round
    for ci, (c, n, l, d, only) in enumerate(cases):
        H, K, m, method = c
        theta, blob, x, t, start, ubar, u_ref, Y_ref, leaves = _fused_oracle(H, K, m, d, n, l, method, 4000 + 10 * ci)
        mid = KN.method_id(method)
        rows, cols, P = KN.ode_act_rows(mid, H, K, m), KN.ode_act_cols(n), blob.numel()
        arena = G.Arena(torch.device(DEVICE))
        tc, bc = arena.inp(t, name='t'), arena.inp(blob, name='theta')
        xT, st, ub = arena.inp(x.t(), name='xT'), arena.inp(start, name='start'), arena.inp(ubar.t(), name='ubar')
        fl = only or SI.forms_of(*c)
        fwd = {}
        tag = '%dx%d-m%d-%s-n%d/' % (H, K, m, method, n)
        for f in fl:
            if f in SI.FWD_FORMS:
                spec = SI.FWD_FORMS[f]
                job = dict(xT=xT, start=st, u=arena.out(l, n, name=f + '.u'), Y=arena.out(l, H, n, name=f + '.Y'))
                if spec['store'] is not None:
                    job['act'] = arena.out(l - 1, rows, cols, name=f + '.act')
                KN.ode_fwd_multi([job], tc, bc, mid, H, K, m, act_x_only=spec['store'] == 'x', narrow=spec['narrow'])
                fwd[f] = job
        sweeps = {}
        for f in fl:
            if f in SI.BWD_FORMS:
                spec = SI.BWD_FORMS[f]
                j = dict(fwd[spec['producer']], ubar=ub, gx=arena.out(d, n, name=f + '.gx'), gs=arena.out(n, name=f + '.gs'))
                if spec['params']:
                    j['gslab'] = arena.out(KN.ode_bwd_slabs(n), P, name=f + '.gslab')
                KN.ode_bwd_multi([j], tc, bc, mid, H, K, m, want_x=True, want_params=spec['params'], adjoint=spec['adjoint'],
                                 narrow=spec['narrow'])
                sweeps[f] = j
        torch.cuda.synchronize()
        for f, job in fwd.items():
            for k in ('u', 'Y', 'act'):
                if k in job:
                    put(tag + f + '.' + k, job[k].view(torch.int64))      # (bits: the untouched parts of a store hold the arena's pattern)
        for f, j in sweeps.items():
            for k in ('gx', 'gs', 'gslab'):
                if k in j:
                    put(tag + f + '.' + k, j[k].view(torch.int64))


def substeps():
    import configs.Ex4_1_funcs as P
    from src.dataset import Comb_loader
    from src.training import NODE_WAN_solver
    nets = (((20, 10, 8), 'midpoint', False), ((32, 12, 3), 'midpoint', False), ((64, 16, 10), 'midpoint', False), ((64, 16, 10), 'euler', False),
            ((32, 12, 3), 'rk4', False), ((20, 10, 8), 'midpoint', True))
    for (H, K, m), solver, adjoint in nets:
        params = {'alpha': 1e8, 'u_layers': m, 'u_hidden_dim': H, 'u_hidden_hidden_dim': K, 'v_layers': 9, 'v_hidden_dim': 50,
                  'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': adjoint, 'solver': solver,
                  'dim': 6, 'N_t': 8, 'N_r': 272, 'N_b': 144, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 1,
                  'domain': 'Hypercube'}
        torch.manual_seed(0)
        S = NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, torch.device('cuda:0'), './',
                            func_u_sol=P.func_u_sol, p=2)
        s = S.setup
        domain = S.domain(s['shape_param'], s['dim'], s['T0'], s['T'], s['N_t'])
        pts = Comb_loader(s['N_r'], s['N_b'], domain, S.device)
        G = S.engine.load_group(pts.interioru, pts.interiorv, pts.boundary, domain)
        tag = 'substeps-%dx%d-m%d-%s%s/' % (H, K, m, solver, '-adjoint' if adjoint else '')
        for i, kind in enumerate('ggdgd'):
            (S.engine.generator_step if kind == 'g' else S.engine.discriminator_step)(G)
            torch.cuda.synchronize()
            put(tag + '%d%s.theta' % (i, kind), S.engine.theta.data)
            put(tag + '%d%s.phi' % (i, kind), S.engine.phi.data)
            put(tag + '%d%s.scal' % (i, kind), S.engine.scal)
        out[tag + 'schedule'] = 'merged=%s compact_tiles=%s graphs=%s G.merged=%s' % (S.engine.merged_sweep, S.engine.compact_tiles,
                                                                                     getattr(S.engine, 'use_graphs', None), getattr(G, 'merged', None))


if len(sys.argv) > 2 and sys.argv[2] == 'forms':
    forms()
substeps()
json.dump(out, open(sys.argv[1], 'w'), indent=0, sort_keys=True)
print('digests:', len(out), sys.argv[1])
