"""The engine on the tiled stepper family (csrc/xw_tiled.hip): generator and discriminator sub-steps against the oracle at widths
only the tiled family serves, a cone-domain group on both families where both run, train() and main.py at such widths, and the
refusals of what the family does not serve."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import configs.Ex4_1_funcs as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = dict(h=P.func_h, f=P.func_f, g=P.func_g, a=P.func_a, b=P.func_b, c=P.func_c)


def _params(Hh, Kk, m, d=5, solver='midpoint', domain='Hypercube', **kw):
    p = {'alpha': 1e3, 'u_layers': m, 'u_hidden_dim': Hh, 'u_hidden_hidden_dim': Kk, 'v_layers': 4, 'v_hidden_dim': 50,
         'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': solver,
         'dim': d, 'N_t': 7, 'N_r': 75, 'N_b': 41, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 1, 'domain': domain}
    p.update(kw)
    return p


def _solver(params, seed, options=None):
    from src.training import NODE_WAN_solver
    torch.manual_seed(seed)
    np.random.seed(seed)
    return NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, torch.device('cuda'), './',
                           func_u_sol=P.func_u_sol, p=2, options=options)


def close(a, b, rtol, atol=0.0, what=''):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=what)


@pytest.mark.parametrize('solver', ['midpoint', 'rk4'])
def test_engine_substeps_on_the_tiled_family_match_the_oracle(solver):
    """(128, 32, 8), d = 5 on the cube: the gradient Adam sees and the parameters after Adam, generator and discriminator
    sub-steps, with the tolerances of tests/test_gpu_engine.py (test_engine_at_other_network_widths)"""
    from oracle import refspec as R
    from src.dataset import Comb_loader
    params = _params(128, 32, 8, solver=solver)
    S = _solver(params, 9)
    eng = S.engine
    assert eng.stepper == 'tiled' and (eng.H, eng.K) == (128, 32) and not eng.use_runner and not eng.keep_activations
    assert eng.use_graphs and eng.use_streams
    assert 'tiled' in S.plan()['stepper']
    torch.manual_seed(9)
    O = R.Solver(params, FUNCS, u_sol=P.func_u_sol, p=2)
    unames = R.u_names(8)
    for n_, k_ in unames:
        assert torch.equal(dict(S.u_net.named_parameters())[n_].detach().cpu(), O.theta[k_]), n_
    rng = torch.get_rng_state()
    s = S.setup
    domain = S.domain(s['shape_param'], s['dim'], s['T0'], s['T'], s['N_t'])
    pts = Comb_loader(s['N_r'], s['N_b'], domain, S.device)
    torch.set_rng_state(rng)
    O.new_sample()
    G = eng.load_group(pts.interioru, pts.interiorv, pts.boundary, domain)
    for step in ('u', 'u', 'v', 'u'):
        if step == 'u':
            o = O.generator_step()
            eng.generator_step(G)
            got, blob, names = eng.grad_u, eng.theta, unames
            close(eng.scal[4], o['loss'], 1e-7)
        else:
            o = O.discriminator_step()
            eng.discriminator_step(G)
            got, blob, names = eng.grad_v, eng.phi, R.V_NAME_MAP
            close(eng.scal[5], o['loss'], 1e-6, 1e-6)
        gmax = max(float(o['grad'][k].abs().max()) for _, k in names)
        for (n_, k_), g_ in zip(names, blob.split(got)):
            close(g_, o['grad'][k_], 1e-5, 1e-6 * gmax, 'grad ' + k_)
    # (atol 1e-6: entries whose gradient is ~1e-8 -- biases of units the ReLUs keep shut on almost every path -- take Adam steps
    #  set by eps = 1e-8, where the rounding of the gradient shows at 1e-7)
    for (n_, k_), p_ in zip(unames, eng.theta.params):
        close(p_, O.theta[k_], 1e-6, 1e-6, 'theta after the updates: ' + k_)
    # the module path (custom operators) at these widths, forward and backward
    X = pts.interioru.detach().clone().requires_grad_(True)
    out = S.u_net(X)
    close(out.squeeze(2), R.u_net(O.theta, params, O.X, P.func_h(O.X[:, 0, :])), 1e-5, 1e-7)
    out.sum().backward()
    assert torch.isfinite(X.grad).all() and all(torch.isfinite(p.grad).all() for p in S.u_net.parameters())


def _cone_run(Hh, Kk, m, options):
    """three sub-steps over the groups of one cone sample: the losses, gradients and parameters after each group"""
    from src.dataset import Comb_loader
    params = _params(Hh, Kk, m, d=3, solver='midpoint', domain='NSphere_TCone', shape_param=1.0, N_r=120, N_b=80, alpha=1e2)
    S = _solver(params, 5, options)
    s = S.setup
    domain = S.domain(s['shape_param'], s['dim'], s['T0'], s['T'], s['N_t'])
    pts = Comb_loader(s['N_r'], s['N_b'], domain, S.device)
    eng = S.engine
    groups = [eng.load_group(pts.interioru[k], pts.interiorv[k], pts.boundary[k], domain)
              for k in range(min(len(pts.interioru), len(pts.boundary)))]
    out = []
    for which in ('u', 'v', 'u'):
        eng.begin_substep(which, True)
        for G in groups:
            G.persistent = False
            (eng.generator_step if which == 'u' else eng.discriminator_step)(G)
            out += [float(eng.scal[4 if which == 'u' else 5]), (eng.grad_u if which == 'u' else eng.grad_v).clone(),
                    eng.theta.data.clone(), eng.phi.data.clone()]
    return eng, out


def test_cone_group_substeps_agree_between_the_tiled_and_generic_families():
    """one cone-domain sample (groups of different lengths, late-entry and single-slice groups, the gradient carried over the
    groups): the tiled family (tiled_stepper = 'generic') against the generic path at (48, 16, 11)"""
    from xnode_wan_pde_solver_amd.options import EngineOptions
    eg, ref = _cone_run(48, 16, 11, EngineOptions())
    et, got = _cone_run(48, 16, 11, EngineOptions(tiled_stepper='generic'))
    assert eg.stepper == 'generic' and et.stepper == 'tiled'
    assert len(ref) == len(got) > 8
    for i, (a, b) in enumerate(zip(got, ref)):
        close(a, b, 1e-9, 1e-12, 'item %d' % i)


def test_cone_group_substeps_run_at_tiled_only_widths():
    from xnode_wan_pde_solver_amd.options import EngineOptions
    eng, out = _cone_run(96, 32, 4, EngineOptions())
    assert eng.stepper == 'tiled'
    for v in out:
        assert np.isfinite(v).all() if not torch.is_tensor(v) else torch.isfinite(v).all()


def _train(tmp_path, seed, graphs):
    """three outer iterations of the synchronous loop (samples drawn in the loop, a read-back after every sub-iteration)"""
    from xnode_wan_pde_solver_amd.options import EngineOptions
    params = _params(128, 32, 8, d=5, solver='midpoint', iterations=3, N_r=200, N_b=100)
    S = _solver(params, seed, EngineOptions(use_graphs=graphs))
    S.pipeline = S.overlap_sampling = False
    tmp_path.mkdir()
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        losses = S.train(report=False)
    finally:
        os.chdir(cwd)
    return list(losses), S.engine.theta.data.clone(), S.engine.phi.data.clone()


def test_train_on_the_tiled_family_is_finite_and_reproducible(tmp_path):
    """three outer iterations of train() on eager launches, twice, after different contents were left in the allocator's cache:
    all six losses and the final theta and phi bit for bit.  With the sub-steps captured as graphs: finite, and the first two
    outer iterations the same as eager.  (From the third outer iteration on, graph-captured training on the slow stepper
    families -- the generic path at (48, 16, 11) as well -- departs from eager launches: DESIGN section 8, tools/train_graph_repro.py.)"""
    junk = torch.full((1 << 24,), float('nan'), dtype=torch.float64, device='cuda')
    del junk
    a = _train(tmp_path / 'a', 4, False)
    junk = torch.full((1 << 24,), 1.0, dtype=torch.float64, device='cuda')
    del junk
    b = _train(tmp_path / 'b', 4, False)
    assert len(a[0]) == 6 and all(np.isfinite(a[0]))
    assert a[0] == b[0]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert torch.isfinite(a[1]).all() and torch.isfinite(a[2]).all()
    c = _train(tmp_path / 'c', 4, True)
    assert len(c[0]) == 6 and all(np.isfinite(c[0])) and torch.isfinite(c[1]).all() and torch.isfinite(c[2]).all()
    assert c[0][:4] == a[0][:4]


def test_main_runs_the_cube_yaml_with_a_wide_field(tmp_path):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'cube_pde.yaml')))
    cfg.update(u_hidden_hidden_dim=32, N_r=400, N_b=400)
    path = tmp_path / 'wide.yaml'
    path.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '--params', str(path), '--funcs', 'Ex4_1_funcs',
                        '-w', str(tmp_path), '--iterations', '3', '--report', '0'], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_refusals_name_their_limits():
    from xnode_wan_pde_solver_amd._lib import XnwanError
    with pytest.raises(XnwanError, match='adjoint=True'):
        _solver(_params(128, 32, 8, adjoint=True), 1)
    with pytest.raises(XnwanError, match="dopri5"):
        _solver(_params(128, 32, 8, solver='dopri5'), 1)
