"""solver 'dopri5' on the tiled stepper family (EngineOptions.dopri5_stepper = 'tiled', csrc/xw_tdopri.hip) in the training engine
(cube domain, one GPU), at (128, 32, 8) -- beyond the vector implementation's widths -- and at the fused container (20, 10, 8): a
generator and a discriminator sub-step against the oracle's sub-steps with its integrator replaced by the dopri5 restatement on
the engine's own accepted grids, train() finite and bit-reproducible, main.py with XW_DOPRI5_STEPPER=tiled, and the refusals that
stay."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dopri5_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _params(**kw):
    p = {'alpha': 1e8, 'u_layers': 8, 'u_hidden_dim': 20, 'u_hidden_hidden_dim': 10, 'v_layers': 9, 'v_hidden_dim': 50,
         'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'dopri5',
         'dim': 4, 'N_t': 8, 'N_r': 96, 'N_b': 96, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 1, 'domain': 'Hypercube'}
    p.update(kw)
    return p


WIDE = dict(u_hidden_dim=128, u_hidden_hidden_dim=32)


def _solver(params, path='./'):
    import configs.Ex4_1_funcs as P
    from src.training import NODE_WAN_solver
    from xnode_wan_pde_solver_amd.options import EngineOptions
    return NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, torch.device('cuda:0'), path,
                           func_u_sol=P.func_u_sol, p=2, options=EngineOptions(dopri5_stepper='tiled'))


def _replay(records):
    """oracle.refspec.odeint_fixed replaced by the dopri5 restatement on the grid the engine's forward accepted for the same
    odeint call (matched by its lifted start state): the constant-step-size semantics of the kernels' sweeps, on the
    device's grid -- a ReLU field's step sequence is not a smooth function of the rounding (tests/test_gpu_dopri5.py)"""
    def odeint(f, y0, t, method):
        assert method == 'dopri5'
        for y0_dev, steps in records:
            if y0_dev.shape == y0.shape and torch.allclose(y0.detach(), y0_dev, rtol=1e-10, atol=1e-13):
                return D.dopri5(f, y0, t.to(F64), count=y0.numel(), frozen=steps)[0]
        raise AssertionError('no dopri5 forward of the engine started from this state')
    return odeint


def _records(engine):
    H = engine.config['u_hidden_dim']
    return [(r.rec_y[0, :H, :].t().cpu().clone(), list(r.steps)) for r in engine._dopri_recs.values()]


def _close(got, want, what, tol=1e-9):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max()) / scale
    assert err < tol, '%s: %.3e' % (what, err)


@pytest.mark.parametrize('widths', [WIDE, {}], ids=['128x32x8', '20x10x8'])
def test_generator_and_discriminator_substeps_against_the_oracle(monkeypatch, widths):
    import configs.Ex4_1_funcs as P
    from oracle import refspec as R
    from src.dataset import Comb_loader
    params = _params(**widths)
    funcs = dict(h=P.func_h, f=P.func_f, g=P.func_g, a=P.func_a, b=P.func_b, c=P.func_c)
    torch.manual_seed(0)
    S = _solver(params)
    assert S.engine.dopri5 and not S.engine.use_graphs and not S.engine.use_runner
    assert S.engine.dopri5_stepper == 'tiled' and S.engine.tiled == bool(widths)
    plan = S.plan()
    assert plan['ode_solver'].startswith('dopri5') and "dopri5_stepper = 'tiled'" in plan['ode_solver'] and 'xw_tdopri.hip' in plan['ode_solver']
    assert plan['options_not_at_their_defaults'] == {'dopri5_stepper': 'tiled'}
    torch.manual_seed(0)
    O = R.Solver(params, funcs, u_sol=P.func_u_sol, p=2)
    s = S.setup
    rng = torch.get_rng_state()
    domain = S.domain(s['shape_param'], s['dim'], s['T0'], s['T'], s['N_t'])
    pts = Comb_loader(s['N_r'], s['N_b'], domain, S.device)
    torch.set_rng_state(rng)
    O.new_sample()
    assert torch.equal(O.X, pts.interioru.detach())
    G = S.engine.load_group(pts.interioru, pts.interiorv, pts.boundary, domain)

    S.engine.generator_step(G)
    torch.cuda.synchronize()
    recs = _records(S.engine)
    assert len(recs) == 2                                                  # interior and boundary: one odeint call each
    assert all(r.stepper == 'tiled' for r in S.engine._dopri_recs.values())
    assert all(len(steps) >= 1 for _, steps in recs)
    monkeypatch.setattr(R, 'odeint_fixed', _replay(recs))
    og = O.generator_step()
    _close(float(S.engine.scal[4]), float(og['loss']), 'loss_u')
    for (name, key), got in zip(R.u_names(8), S.engine.theta.params):
        _close(got.detach().cpu().numpy(), O.theta[key].numpy(), name)

    S.engine.discriminator_step(G)
    torch.cuda.synchronize()
    monkeypatch.setattr(R, 'odeint_fixed', _replay(_records(S.engine)))
    od = O.discriminator_step()
    # the discriminator sub-step at the bound of the fixed-grid oracle comparisons (tests/test_gpu_engine.py, smoke()): the
    # reference keeps nabla u / nabla phi in float32 .grad tensors, the engine in float64
    _close(float(S.engine.scal[5]), float(od['loss']), 'loss_v', 1e-6)
    for (name, key), got in zip(R.V_NAME_MAP, S.engine.phi.params):
        _close(got.detach().cpu().numpy(), O.phi[key].numpy(), name, 1e-6)
    assert np.isfinite(float(S.engine.predict(pts.interioru).abs().max()))


def _train_once(tmp_path, sub):
    d = tmp_path / sub
    d.mkdir()
    cwd = os.getcwd()
    os.chdir(d)
    try:
        torch.manual_seed(3)
        S = _solver(_params(iterations=3, **WIDE), str(d) + '/')
        S.train()
        torch.cuda.synchronize()
        return S.engine.theta.data.detach().cpu().clone(), S.engine.phi.data.detach().cpu().clone()
    finally:
        os.chdir(cwd)


def test_train_three_iterations_finite_and_reproducible(tmp_path):
    th1, ph1 = _train_once(tmp_path, 'a')
    th2, ph2 = _train_once(tmp_path, 'b')
    assert bool(torch.isfinite(th1).all()) and bool(torch.isfinite(ph1).all())
    assert torch.equal(th1, th2) and torch.equal(ph1, ph2)


def test_the_cone_domain_and_the_adjoint_still_raise():
    from xnode_wan_pde_solver_amd._lib import XnwanError
    for widths in (WIDE, {}):
        with pytest.raises(XnwanError, match='cube domain only'):
            _solver(_params(domain='NSphere_TCone', **widths))
        with pytest.raises(XnwanError, match="'dopri5' with adjoint=True"):
            _solver(_params(adjoint=True, **widths))


def test_main_with_a_wide_dopri5_yaml(tmp_path):
    """main.py on the shipped cube YAML with `solver: 'dopri5'` at (128, 32) (a small sample), in a child process with
    XW_DOPRI5_STEPPER=tiled in its environment; without the variable the same YAML is refused, naming the option"""
    import subprocess
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'configs', 'cube_pde.yaml')) as fh:
        params = yaml.safe_load(fh)
    params.update(solver='dopri5', N_r=128, N_b=128, N_t=8, **WIDE)
    cfg = tmp_path / 'cube_dopri5.yaml'
    cfg.write_text(yaml.safe_dump(params))
    cmd = [sys.executable, os.path.join(root, 'main.py'), '--params', str(cfg), '--funcs', 'Ex4_1_funcs',
           '-w', str(tmp_path) + '/', '--iterations', '2', '--report', 'false']
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('XW_DOPRI5_STEPPER', None)
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode != 0 and 'dopri5_stepper' in r.stdout + r.stderr
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600, env=dict(env, XW_DOPRI5_STEPPER='tiled'))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / 'losses_NODE_5.json').exists()
