"""tools/sample_digests.py OUT.json -- SHA-256 of what each of the engine's four group loaders leaves in a group, and of the parameters
one outer iteration on top of it gives, for comparing two trees bit by bit (profiles/r26_group_loading.md): run it once per tree, one
fresh process each, and compare the JSON files on the host.  Seeded, a few seconds.  Per loaded group: every Group.SAMPLE_FIELDS
tensor (or None), the scalars, has_bdry, sharded and the names of the work buffers; per case theta, phi and the scalar block after two
generator and one discriminator sub-iteration.  Cases: the cube (d = 5, N_t = 9, 300 + 140 paths) through load_group from host tensors,
from device tensors over one shared grid, through refill_compact's lean body and -- with the general coefficients of
tests/golden/general_funcs.py -- its general body; the cone and the hourglass through solver._prepare_groups, group by group and by
one gather launch; Engine.predict and solver._l_norm on the first sample of the cube and of the cone."""
import hashlib
import importlib.util
import json
import os
import sys
import types
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

out = {}
BASE = {'alpha': 1e8, 'u_layers': 8, 'u_hidden_dim': 20, 'u_hidden_hidden_dim': 10, 'v_layers': 9, 'v_hidden_dim': 50, 'n1': 2, 'n2': 1,
        'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'midpoint', 'T0': 0, 'T': 1, 'iterations': 1}
CUBE = dict(BASE, dim=5, N_t=9, N_r=300, N_b=140, shape_param=[-1, 1], domain='Hypercube')
BALL = dict(BASE, alpha=1e4, dim=5, N_t=9, N_r=1500, N_b=700, shape_param=1.0)


def put(name, t):
    if t is None:
        out[name] = None
        return
    t = t.detach().contiguous().cpu()
    out[name] = '%s %s %s' % (hashlib.sha256(t.numpy().tobytes()).hexdigest(), str(t.dtype), list(t.shape))


def solver(params, seed, F):
    from src.training import NODE_WAN_solver
    torch.manual_seed(seed)
    np.random.seed(seed)
    return NODE_WAN_solver(params, F.func_a, F.func_b, F.func_c, F.func_h, F.func_f, F.func_g, torch.device('cuda'), './',
                           func_u_sol=F.func_u_sol, p=2)


def general(base):
    spec = importlib.util.spec_from_file_location('general_funcs', os.path.join(ROOT, 'tests', 'golden', 'general_funcs.py'))
    GF = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(GF)
    return types.SimpleNamespace(func_a=GF.func_a, func_b=GF.func_b, func_c=GF.func_c, func_h=base.func_h, func_f=base.func_f,
                                 func_g=base.func_g, func_u_sol=base.func_u_sol)


def put_groups(tag, groups):
    from xnode_wan_pde_solver_amd.engine import Group
    torch.cuda.synchronize()
    out[tag + 'groups'] = len(groups)
    for i, G in enumerate(groups):
        for k in Group.SAMPLE_FIELDS:
            put('%sG%02d.%s' % (tag, i, k), getattr(G, k, None))
        out['%sG%02d.meta' % (tag, i)] = repr((G.N, G.L, G.Nb, G.Lb, G.same_grid, G.Vol, G.Nglob, G.Nbglob, G.pair_i, G.pair_b, G.init_off,
                                               G.bdry_off, G.s3_scale, G.amode, G.has_bdry, G.sharded, G.sample_version))
        out['%sG%02d.lazy' % (tag, i)] = sorted(G._lazy)


def outer_iteration(tag, S, groups):
    eng, many = S.engine, len(groups) > 1
    for G in groups:
        G.persistent = False
    for which, count, step in (('u', 2, eng.generator_step), ('v', 1, eng.discriminator_step)):
        for _ in range(count):
            eng.begin_substep(which, many)
            for G in groups:
                step(G)
    torch.cuda.synchronize()
    put(tag + 'theta', eng.theta.data)
    put(tag + 'phi', eng.phi.data)
    put(tag + 'scal', eng.scal)


def cube_sample(S):
    from src.dataset import Comb_loader
    s = S.setup
    dom = S.domain(s['shape_param'], s['dim'], s['T0'], s['T'], s['N_t'])
    return dom, Comb_loader(s['N_r'], s['N_b'], dom, S.device)


def on_device(S, comp):
    from xnode_wan_pde_solver_amd import sampling
    td = comp[0].to(S.device)
    return [sampling._paths(td, c.to(S.device)) for c in comp[1:]]


def cube_cases():
    import configs.Ex4_1_funcs as P
    S = solver(CUBE, 5, P)
    dom, pts = cube_sample(S)
    G = S.engine.load_group(pts.interioru, pts.interiorv, pts.boundary, dom)
    put_groups('cube-host/', [G])
    put('cube-host/predict', S.engine.predict(pts.interioru))
    out['cube-host/l_norm'] = repr(float(S._l_norm(pts, dom.V())))
    outer_iteration('cube-host/', S, [G])

    S = solver(CUBE, 5, P)
    dom, pts = cube_sample(S)
    comp = pts.compact()
    G = S.engine.load_group(*on_device(S, comp), dom, shared_grid_t0=float(comp[0][0]))
    put_groups('cube-device/', [G])
    put('cube-device/predict', S.engine.predict(on_device(S, comp)[0]))
    out['cube-device/l_norm'] = repr(float(S._l_norm(pts, dom.V())))
    outer_iteration('cube-device/', S, [G])

    for name, F in (('lean', P), ('general', general(P))):
        S = solver(CUBE, 5, F)
        tag = 'cube-refill-%s/' % name
        dom, pts = cube_sample(S)
        comp = pts.compact()
        G = S.engine.load_group(*on_device(S, comp), dom, shared_grid_t0=float(comp[0][0]))
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)       # (a body that cannot be captured runs eagerly, with a warning)
            for rep in range(3):                                   # the capture pass and two replays, a new sample each
                dom, pts = cube_sample(S)
                assert S.engine.refill_compact(G, pts.compact(), dom) is G
                put_groups('%s%d/' % (tag, rep), [G])
        out[tag + 'graphs'] = sorted('%s: %s' % (k.split('_')[0], type(v).__name__) for k, v in G.graphs.items() if k.startswith('refill'))
        outer_iteration(tag, S, [G])


def ball_cases():
    import configs.Ex4_3_funcs as F
    for domain, seed in (('NSphere_TCone', 6), ('NSphere_THourglass', 5), ('NSphere_THourglass', 8), ('NSphere_TCone', 9)):
        for packed in (True, False):
            S = solver(dict(BALL, domain=domain), seed, F)
            S.engine.packed_load = packed
            tag = '%s-%d-%s/' % (domain, seed, 'packed' if packed else 'by-group')
            dom = S._new_domain()
            pts = S._loader(dom).pin()
            groups = S._prepare_groups(pts, dom)
            put_groups(tag, groups)
            out[tag + 'by one gather launch'] = all('xT' in G._lazy for G in groups)
            if (domain, seed) == ('NSphere_TCone', 6):
                for i, (X, _, _) in enumerate(S._groups(pts)):
                    put('%spredict%02d' % (tag, i), S.engine.predict(X))
                out[tag + 'l_norm'] = repr(float(S._l_norm(pts, dom.V())))
            outer_iteration(tag, S, groups)


cube_cases()
ball_cases()
json.dump(out, open(sys.argv[1], 'w'), indent=0, sort_keys=True)
print('digests:', len(out), sys.argv[1])
