"""The module autograd surface on the device: `u_net(X)`, `v_net(XV)`, `.backward()`, the `loss` class and the torch optimisers --
nets._OdeFn / _Dopri5Fn / _DiscFn, XNODE.forward with its single-slice and bound_pad branches, the operators of ops.py, Blob.split and
compat_loss.loss, i.e. the host marshalling between a user and the kernels.

  A  a reference sub-iteration through the modules (make_golden.net_step, its order and leaves) on the cube fixtures: gen1, gen2, disc1
     against the vectors recorded from the reference's own modules and loss, at the tolerances of test_gpu_engine._first_iteration.check
     (float32 resolution downstream of the float32 callables; gradients 1e-5 relative to the largest gradient entry: that file's header).
  B  the same on the list domains, in the reference's loop order over the fixture's pairs, group 0 -- the single-slice pairwise group --
     included; which parameters have no gradient and Adam's step counts compared exactly.
  C  the edge matrix of tests/module_surface.py against the oracle (float64 on both sides), the single-slice and bound_pad branches,
     the refusals.

The time channel of X's gradient is returned as zero by this project (nets._OdeFn.backward): asserted; the fixtures' `Xgrad_t_path0`
(non-zero on path 0 in the reference, never read by the loss) is deliberately not reproduced.
"""
import atexit
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import module_surface as M  # noqa: E402
import test_gpu_engine as E  # noqa: E402
from test_gpu_engine import F32TOL, first_sample, load, make_solver, thin  # noqa: E402

import configs.Ex4_1_funcs as P  # noqa: E402

pytestmark = pytest.mark.gpu

CUBE_CASES = [c for c in E.CASES if c != 'ref_d20_headline']      # (a slim record of 4096 paths: the compat loss would tabulate a 420 MB `a`)
WIDE_CASES = ['ref_wide_testnet_d4_midpoint', 'ref_wide_testnet_d3_rk4', 'ref_wide_testnet_both_d5_euler']
GROUP_CASES = ['ref_cone_groups', 'ref_hourglass_groups', 'ref_cone_ex43_d10_groups', 'ref_hourglass_ex43_d10_groups', 'ref_cone_r07_groups',
               'ref_cone_general_groups', 'ref_hourglass_general_groups', 'ref_cone_alpha1_groups', 'ref_hourglass_alpha1_groups',
               'ref_hourglass_alpha1_general_groups', 'ref_hourglass_const_a_groups']

# the largest observed error of every compared quantity as a fraction of its bound (profiles/r22_module_surface.md); written to the
# file XW_SURFACE_STATS names, if set
WORST = {}


def close(part, what, a, b, rtol, atol=0.0):
    a, b = E._np(a), E._np(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    frac = float(np.max(np.abs(a - b) / (atol + rtol * np.abs(b) + 1e-300))) if a.size else 0.0
    WORST[part + ' ' + what] = max(WORST.get(part + ' ' + what, 0.0), frac)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=part + ' ' + what)


@atexit.register
def _dump():
    if os.environ.get('XW_SURFACE_STATS') and WORST:
        with open(os.environ['XW_SURFACE_STATS'], 'w') as fh:
            json.dump(WORST, fh, indent=1, sort_keys=True)


def _general(golden_dir):
    import importlib.util
    spec = importlib.util.spec_from_file_location('general_funcs', os.path.join(golden_dir, 'general_funcs.py'))
    GF = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(GF)
    return GF


def _fresh(t):
    return t.detach().clone().requires_grad_(True)


# ---- A: cube fixtures ----------------------------------------------------------------------------------------------------------
def _sub_iteration_through_the_modules(golden_dir, fixture_dir, case):
    import types
    from src.loss import loss
    from src.training import func_eval
    z, params = load(fixture_dir, case)
    fname = str(params.pop('funcs', ''))
    F = P
    if fname.startswith('general_'):                      # the callables the fixture was recorded with, as _first_iteration loads them
        fa, fb, fc = _general(golden_dir).variant(fname[len('general_'):])
        F = types.SimpleNamespace(func_a=fa, func_b=fb, func_c=fc, func_h=P.func_h, func_f=P.func_f, func_g=P.func_g, func_u_sol=P.func_u_sol)
    S = make_solver(params, int(z['seed']), F=F)
    domain, pts = first_sample(S)

    def net_step(tag, which, datau, datav, bdata, opt):
        opt.zero_grad()
        pv = S.v_net(datav)
        pu = S.u_net(datau)
        h, f, g, a, b, c = func_eval(datau.clone().detach(), bdata.clone().detach(), S.setup, pu, F.func_a, F.func_b, F.func_c, F.func_h,
                                     F.func_f, F.func_g)
        Lo = loss(S.config['alpha'], a, b, c, h, f, g, S.setup, domain, S.device)
        # the input gradients the way the fixture took them (side-effect free)
        G = torch.autograd.grad(pu.sum(), datau, retain_graph=True)[0]
        w = domain.func_w(datav).unsqueeze(2)
        dphi = torch.autograd.grad((pv * w.to(pv.device)).sum(), datav, retain_graph=True)[0]
        assert G.dtype == datau.dtype and G.device == datau.device and dphi.dtype == datav.dtype and dphi.device == datav.device
        close('A', 'u', thin(z, pu.squeeze(2)), z[tag + '/u'], F32TOL, F32TOL)
        first = tag == 'gen1'
        close('A', 'v (initial phi)' if first else 'v', thin(z, pv.squeeze(2)), z[tag + '/v'], 1e-10 if first else F32TOL, 1e-12 if first else F32TOL)
        close('A', 'nabla_x u', thin(z, G[:, 0, 1:]), z[tag + '/Xgrad_l0'][:, 1:], 2e-5, 1e-6)
        assert float(G[:, :, 0].abs().max()) == 0.0, 'the time channel of d(sum u)/dX is returned as zero'
        if G.shape[1] > 1:
            assert float(G[:, 1:, 1:].abs().max()) == 0.0
        close('A', 'dphi (time channel included)', thin(z, dphi, 4), z[tag + '/dphi'], 2e-5, 1e-6)
        if which == 'u':
            close('A', 'init', Lo.init(pu), float(z[tag + '/init']), 1e-5)
            close('A', 'bdry', Lo.bdry(S.u_net, bdata), float(z[tag + '/bdry']), 1e-5)
            L = Lo.u(pu, pv, S.u_net, datau, datav, bdata)
        else:
            L = Lo.v(pu, pv, datau, datav)
        close('A', 'loss_' + which, L, float(z[tag + '/loss']), 1e-5)
        # the .grad side effects the compat loss documents: X.grad and XV.grad are left zeroed (the generator's p.grad holds
        # d(sum u)/dtheta from the helper backward pass: part of the recorded gradient below)
        assert float(datau.grad.abs().max()) == 0.0 and float(datav.grad.abs().max()) == 0.0
        L.backward()
        net = S.u_net if which == 'u' else S.v_net
        names = [n for n, _ in net.named_parameters()]
        gmax = max(float(np.abs(z[tag + '/grad/' + n]).max()) for n in names)
        for n, p in net.named_parameters():
            assert p.grad is not None and p.grad.shape == p.shape, n
            close('A', 'grad_' + which, p.grad, z[tag + '/grad/' + n], 1e-5, 1e-6 * gmax)
        opt.step()
        for n, p in net.named_parameters():
            close('A', 'after_' + which, p, z[tag + '/after/' + n], 1e-5, 1e-7)

    datau, datav, bdata = pts.interioru, pts.interiorv, pts.boundary        # gen1: the loader's own host leaves
    net_step('gen1', 'u', datau, datav, bdata, S.optimizer_u)
    net_step('gen2', 'u', _fresh(pts.interioru), _fresh(pts.interiorv), _fresh(pts.boundary), S.optimizer_u)
    net_step('disc1', 'v', _fresh(pts.interioru), _fresh(pts.interiorv), _fresh(pts.boundary), S.optimizer_v)


@pytest.mark.parametrize('case', CUBE_CASES)
def test_reference_sub_iteration_through_the_modules(golden_dir, case):
    _sub_iteration_through_the_modules(golden_dir, golden_dir, case)


@pytest.mark.parametrize('case', WIDE_CASES)
def test_reference_sub_iteration_through_the_modules_with_a_tiled_test_network(golden_dir, tmp_path, case):
    from test_gpu_tiled_testnet_engine import expand
    _sub_iteration_through_the_modules(golden_dir, expand(golden_dir, case, tmp_path), case)


# ---- B: list domains -----------------------------------------------------------------------------------------------------------
def _group_callables(golden_dir, params):
    import types
    F = P
    fname = params.pop('funcs', 'Ex4_1_funcs')
    if fname.startswith('Ex4_3_funcs'):
        import configs.Ex4_3_funcs as F
    if fname.endswith('+general_ac'):
        GF = _general(golden_dir)
        F = types.SimpleNamespace(func_a=GF.func_a, func_b=F.func_b, func_c=GF.func_c, func_h=F.func_h, func_f=F.func_f, func_g=F.func_g,
                                  func_u_sol=F.func_u_sol)
    if fname.endswith('+general_const'):
        GF = _general(golden_dir)
        F = types.SimpleNamespace(func_a=GF.const_a, func_b=F.func_b, func_c=GF.lin_c, func_h=F.func_h, func_f=F.func_f, func_g=F.func_g,
                                  func_u_sol=F.func_u_sol)
    return F


@pytest.mark.parametrize('optim', ['fused', 'torch'])
@pytest.mark.parametrize('case', GROUP_CASES)
def test_list_domain_group_loop_through_the_modules(golden_dir, case, optim):
    """zero_grad() once per sub-iteration, optimizer.step() after every group, over the pairs of the fixture; the tolerances of
    test_sphere_domain_groups_against_reference_vectors.  Group 0 is the single-slice group at T0: u_net returns [N, 1], the loss
    forms its [N, N] pairwise terms, the field's parameters have NO gradient (has_grad) and Adam skips them (adam_steps).
    optim: 'fused' -- the solver's own optimizer_u / optimizer_v (solver.FusedAdam, the fused HIP Adam kernel on the blob: its step
    counts are `steps()`); 'torch' -- torch.optim.Adam over the modules' parameters, the views of the blob (its `state`).

    Measured on the parent commit (profiles/r22_module_surface.md): loss.I raised on group 0 (IndexError: Dimension out of range);
    with I mended, _OdeFn.backward gave the field's parameters zero tensors -- at step 0 of ref_cone_groups / ref_hourglass_groups
    1481 of 1481 entries had a gradient where the fixture records 901, so that an optimiser counts a step for them that the
    reference's does not (adam_steps 0)."""
    from src.dataset import Comb_loader
    from src.loss import loss
    from src.training import func_eval
    z, params = load(golden_dir, case)
    F = _group_callables(golden_dir, params)
    S = make_solver(params, int(z['seed']), F=F)
    s = S.setup
    domain = S.domain(s['shape_param'], s['dim'], s['T0'], s['T'], s['N_t'])
    pts = Comb_loader(s['N_r'], s['N_b'], domain, S.device)
    for k, g_ in enumerate(pts.interioru):
        E.close(g_, z['interior/%d' % k], 1e-13, 1e-15, 'interior group %d' % k)
    for k, g_ in enumerate(pts.boundary):
        E.close(g_, z['boundary/%d' % k], 1e-13, 1e-15, 'boundary group %d' % k)
    pairs = [tuple(p) for p in z['pairs']]
    opt_u, opt_v = S.optimizer_u, S.optimizer_v
    if optim == 'torch':
        opt_u = torch.optim.Adam(S.u_net.parameters(), lr=S.config['u_rate'])
        opt_v = torch.optim.Adam(S.v_net.parameters(), lr=S.config['v_rate'])
    assert pts.interioru[0].shape[1] == 1 and pts.interioru[0][0, 0, 0].item() == s['T0']
    step = 0
    for which, opt, net in (('u', opt_u, S.u_net), ('u', opt_u, S.u_net), ('v', opt_v, S.v_net)):
        opt.zero_grad()
        for ki, kb in pairs:
            tag = 'step%d' % step
            assert str(z[tag + '/which']) == which
            datau, datav, bdata = _fresh(pts.interioru[ki]), _fresh(pts.interiorv[ki]), _fresh(pts.boundary[kb])
            pv, pu = S.v_net(datav), S.u_net(datau)
            assert tuple(pu.shape) == ((datau.shape[0], 1) if ki == 0 else tuple(datau.shape[:2]) + (1,))
            h, f, g, a, b, c = func_eval(datau.clone().detach(), bdata.clone().detach(), s, pu, F.func_a, F.func_b, F.func_c, F.func_h,
                                         F.func_f, F.func_g)
            Lo = loss(S.config['alpha'], a, b, c, h, f, g, s, domain, S.device)
            if which == 'u':
                with torch.no_grad():
                    close('B', 'init', Lo.init(pu), float(z[tag + '/init']), 1e-9)
                    close('B', 'bdry', Lo.bdry(S.u_net, bdata), float(z[tag + '/bdry']), 1e-9)
            L = Lo.u(pu, pv, S.u_net, datau, datav, bdata) if which == 'u' else Lo.v(pu, pv, datau, datav)
            assert float(datau.grad.abs().max()) == 0.0 and float(datav.grad.abs().max()) == 0.0
            L.backward()
            close('B', 'u', pu.reshape(pu.shape[0], -1), z[tag + '/u'], 1e-5, 1e-7)
            close('B', 'v', pv.squeeze(2), z[tag + '/v'], 1e-5, 1e-7)
            close('B', 'loss_' + which, L, float(z[tag + '/loss']), 1e-5)
            ps = list(net.parameters())
            has = np.concatenate([np.full(p.numel(), p.grad is not None) for p in ps])
            assert np.array_equal(has, z[tag + '/has_grad']), \
                '%s: %d of %d entries have a gradient, the reference %d' % (tag, int(has.sum()), has.size, int(z[tag + '/has_grad'].sum()))
            grad = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in ps])
            ref = z[tag + '/grad']
            close('B', 'grad_' + which, grad, ref, 1e-5, 1e-6 * float(np.abs(ref).max()))
            opt.step()
            steps = opt.steps() if optim == 'fused' else [int(opt.state[p]['step']) if p in opt.state and 'step' in opt.state[p] else 0 for p in ps]
            assert steps == [int(v) for v in z[tag + '/adam_steps']], '%s: Adam step counts %s, the reference %s' % (tag, steps, list(z[tag + '/adam_steps']))
            close('B', 'after_' + which, torch.cat([p.detach().reshape(-1) for p in ps]), z[tag + '/after'], 1e-5, 1e-7)
            step += 1
    assert step == int(z['n_steps'])


# ---- C: the edge matrix against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', M.U_CASES, ids=M.case_id)
def test_u_net_surface_against_the_oracle(c):
    net = M.run_u_case(c, 'cuda')
    if c.solver == 'dopri5':
        assert net.last_dopri5.stepper == c.stepper


@pytest.mark.parametrize('c', M.U_CASES, ids=M.case_id)
def test_input_gradient_with_every_parameter_frozen_has_the_bits_of_the_full_case(c):
    """only X requires a gradient: d/dX equal bit for bit to d/dX of the full case.

    This test found a defect: while _OdeFn.backward ran the sweep without want_params when every parameter was frozen, case 2 --
    (20, 10, 8), rk4, N = 15, L = 5, d = 1, float64 -- differed from the full case in the last bit of 10 of its 15 non-zero entries
    (8.7e-19, 1.44e-16 of the largest entry): that sweep is another kernel instantiation (k_ode_bwd<.., PARAMS = false>).  The
    Function now always runs the sweep with its parameter part (profiles/r22_module_surface.md)."""
    full, only, n, rel = M.x_only_bits(c, 'cuda')
    assert n == 0, '%d of %d entries differ, by up to %.1e of the largest entry' % (n, full.numel(), rel)


@pytest.mark.parametrize('c', M.V_CASES, ids=M.case_id)
def test_v_net_surface_against_the_oracle(c):
    M.run_v_case(c, 'cuda')


@pytest.mark.parametrize('boundary', [False, True], ids=['at_T0', 'on_the_boundary'])
@pytest.mark.parametrize('shape,solver,stepper,N', M.SLICE_CASES)
def test_single_time_slice(shape, solver, stepper, N, boundary):
    M.run_slice_case(shape, solver, stepper, N, 'cuda', boundary)


def test_evaluation_path_over_a_bound_pad_grid_carries_gradients():
    M.run_bound_pad_case('cuda')


def test_refusals_keep_their_messages():
    M.check_refusals('cuda')
