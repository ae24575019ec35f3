"""The engine with a test network on the tiled family (csrc/xw_disc_tiled.hip): one outer iteration and a trajectory against the
reference's own runs (tests/golden/make_golden_wide_testnet.py), the sub-steps of a cone group, train() and main.py, plan()."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import configs.Ex4_1_funcs as P
from test_gpu_engine import _first_iteration, load, make_solver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def expand(golden_dir, case, out_dir):
    """the full one-iteration file make_golden.py writes, from its compact form (tests/golden/make_golden_wide_testnet.py):
    the large initial parameters from a solver built with the fixture's seed, checked against the reference's SHA-1s; the
    parameters after each optimiser step as before + the reference's float32 step"""
    import hashlib
    z, params = load(golden_dir, case)
    full = dict(z)
    S = make_solver(params, int(z['seed']))
    own = {'u': dict(S.u_net.named_parameters()), 'v': dict(S.v_net.named_parameters())}
    for k in [k for k in full if '_sd_sha1/' in k]:
        tag, name = k.split('_sd_sha1/')
        a = own[tag][name].detach().cpu().numpy().astype(np.float64)
        assert hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest() == str(full.pop(k)), 'initial ' + k
        full[tag + '_sd/' + name] = a
    before = {'gen1': 'u_sd/', 'disc1': 'v_sd/', 'gen2': 'gen1/after/'}
    for tag in ('gen1', 'disc1', 'gen2'):                             # (gen2 starts from gen1's result)
        for k in [k for k in full if k.startswith(tag + '/step/')]:
            name = k[len(tag + '/step/'):]
            full[tag + '/after/' + name] = full[before[tag] + name] + full.pop(k).astype(np.float64)
    np.savez(os.path.join(out_dir, case + '.npz'), **full)
    return str(out_dir)


@pytest.mark.parametrize('case', ['ref_wide_testnet_d4_midpoint', 'ref_wide_testnet_d3_rk4', 'ref_wide_testnet_both_d5_euler'])
def test_first_iteration_matches_the_reference(golden_dir, tmp_path, case):
    _first_iteration(expand(golden_dir, case, tmp_path), case)


def test_trajectory_matches_the_reference(golden_dir, tmp_path):
    """25 outer iterations of train() at u (20, 10, 8) + v (256, 9), d = 3: rel-L2 at every generator sub-step against the
    reference's own run, as for ref_traj_generic_d3_seed14"""
    from utils.auxillary_funcs import rel_err
    z, params = load(golden_dir, 'ref_traj_wide_testnet_d3_seed50')
    ref = z['rel_l2']
    log = []

    def hook(self, pts, domain):
        log.append(float(rel_err(pts, self.u_net, self.func_u_sol, self.p, domain.V(), self.params['N_r'])))
        return False
    S = make_solver(params, int(z['seed']), stop=hook)
    assert S.engine.testnet == 'tiled' and 'tiled' in S.plan()['testnet']
    S.tabulate_on_host = True
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        S.train(report=False)
    finally:
        os.chdir(cwd)
    got = np.array(log)
    assert got.shape == ref.shape == (50,)
    np.testing.assert_allclose(got, ref, rtol=1e-4)


def _params(W, q, d=3, **kw):
    p = {'alpha': 1e2, 'u_layers': 8, 'u_hidden_dim': 20, 'u_hidden_hidden_dim': 10, 'v_layers': q, 'v_hidden_dim': W,
         'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'midpoint',
         'dim': d, 'N_t': 7, 'N_r': 120, 'N_b': 80, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 1, 'domain': 'Hypercube'}
    p.update(kw)
    return p


def test_cone_group_substeps_with_a_wide_test_network():
    """one cone-domain sample at v (256, 9): groups of different lengths, late-entry and single-slice groups (the pairwise form)"""
    from src.dataset import Comb_loader
    params = _params(256, 9, domain='NSphere_TCone', shape_param=1.0)
    S = make_solver(params, 5)
    eng = S.engine
    assert eng.testnet == 'tiled' and not eng.use_runner and eng.xproj_min_d > 128
    s = S.setup
    domain = S.domain(s['shape_param'], s['dim'], s['T0'], s['T'], s['N_t'])
    pts = Comb_loader(s['N_r'], s['N_b'], domain, S.device)
    groups = [eng.load_group(pts.interioru[k], pts.interiorv[k], pts.boundary[k], domain)
              for k in range(min(len(pts.interioru), len(pts.boundary)))]
    assert len(groups) > 2
    phi0 = eng.phi.data.clone()
    for which in ('u', 'v', 'u', 'v'):
        eng.begin_substep(which, True)
        for G in groups:
            G.persistent = False
            (eng.generator_step if which == 'u' else eng.discriminator_step)(G)
            assert np.isfinite(float(eng.scal[4 if which == 'u' else 5]))
            assert torch.isfinite(eng.grad_u).all() and torch.isfinite(eng.grad_v).all()
    assert not torch.equal(phi0, eng.phi.data) and torch.isfinite(eng.phi.data).all()


def _train(tmp_path, seed):
    from xnode_wan_pde_solver_amd.options import EngineOptions
    params = _params(256, 20, d=5, iterations=3, N_r=200, N_b=100)
    S = make_solver(params, seed, options=EngineOptions(use_graphs=False))
    S.pipeline = S.overlap_sampling = False
    tmp_path.mkdir()
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        losses = S.train(report=False)
    finally:
        os.chdir(cwd)
    return S, list(losses), S.engine.theta.data.clone(), S.engine.phi.data.clone()


def test_train_with_a_wide_deep_test_network_is_finite_and_reproducible(tmp_path):
    """v (256, 20): three outer iterations of train() on eager launches, twice, bit for bit"""
    junk = torch.full((1 << 24,), float('nan'), dtype=torch.float64, device='cuda')
    del junk
    S, *a = _train(tmp_path / 'a', 4)
    b = _train(tmp_path / 'b', 4)[1:]
    assert S.engine.testnet == 'tiled'
    assert S.plan()['testnet'].startswith('tiled MFMA family at width 256')
    assert len(a[0]) == 6 and all(np.isfinite(a[0]))
    assert a[0] == b[0]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert torch.isfinite(a[1]).all() and torch.isfinite(a[2]).all()


def test_plan_names_the_test_network_family():
    S = make_solver(_params(50, 9), 1)
    assert S.plan()['testnet'] == 'fused MFMA container 50'
    S = make_solver(_params(128, 17), 1)
    assert S.plan()['testnet'] == 'tiled MFMA family at width 128 (csrc/xw_disc_tiled.hip)'
    assert S.engine.xproj_min_d > 128                               # (no x-projection table, also at a container width)


def test_main_runs_the_cube_yaml_with_a_wide_test_network(tmp_path):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'cube_pde.yaml')))
    cfg.update(v_hidden_dim=256, v_layers=20, N_r=400, N_b=400)
    path = tmp_path / 'wide_v.yaml'
    path.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '--params', str(path), '--funcs', 'Ex4_1_funcs',
                        '-w', str(tmp_path), '--iterations', '3', '--report', '0'], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
