"""The module-surface tests without a GPU (tests/module_surface.py): the case tables cover what they promise; the real modules,
autograd Functions and operators (nets.py, ops.py) over plain-torch stand-ins of the kernel wrappers pass every comparison of
tests/test_gpu_module_surface.py on every case; each planted defect makes the comparison fail; and compat_loss.loss -- plain torch --
is pinned against oracle/refspec.py and the list-domain fixtures, single-slice pairwise group included."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import module_surface as M  # noqa: E402

F64 = torch.float64


# ---- the tables --------------------------------------------------------------------------------------------------------------
def test_case_tables_cover_every_axis_value_and_every_pairing():
    from xnode_wan_pde_solver_amd import kernels as KN
    for cases, pairing in ((M.U_CASES, M.u_pairing), (M.V_CASES, M.v_pairing)):
        for axis, values in (('N', M.NS), ('L', M.LS), ('d', M.DS), ('cot', M.COTS), ('dtype', M.DTYPES), ('place', M.PLACES),
                             ('layout', M.LAYOUTS)):
            assert {getattr(c, axis) for c in cases} == set(values), axis
        met = {(pairing(c), c.cot) for c in cases}
        for key in {pairing(c) for c in cases}:
            assert {(key, k) for k in M.COTS} <= met, key + ' does not meet every cotangent kind'
        assert all(c.N != c.L for c in cases)
    assert {M.u_pairing(c) for c in M.U_CASES} == {'mfma', 'generic', 'tiled', 'mfma+adjoint', 'tiled+adams', 'dopri5/vector', 'dopri5/tiled'}
    assert {M.v_pairing(c) for c in M.V_CASES} == {'mfma', 'tiled'}
    # every requires-grad subset runs inside every case (run_u_case / run_v_case): the pairing with the families is the tables'
    assert M.SUBSETS == ('all', 'x_only', 'params_only', 'one_frozen', 'leaf_twice')
    # the stepper families and solvers
    widths = {M.U_SHAPES[c.shape][:3] for c in M.U_CASES}
    assert {(20, 10, 8), (7, 3, 2), (32, 12, 10), (64, 16, 2), (48, 16, 11), (128, 32, 4), (33, 17, 2)} <= widths
    for s in ('exact20', 'embed7', 'c32', 'c64', 'generic48', 'tiled128', 'tiled33'):
        assert {c.solver for c in M.U_CASES if c.shape == s and not c.adjoint} >= set(M.FIXED), s
    assert any(c.adjoint and M.U_SHAPES[c.shape][3] == 'mfma' for c in M.U_CASES)
    assert any(c.solver == 'explicit_adams' and M.U_SHAPES[c.shape][3] == 'tiled' and c.L == 5 for c in M.U_CASES)
    assert {c.stepper for c in M.U_CASES if c.solver == 'dopri5'} == {'vector', 'tiled'}
    for H, K, m, fam, kdims, _ in M.U_SHAPES.values():
        assert KN.stepper_family(H, K, m) == fam and tuple(KN.stepper_kdims(H, K, m)) == kdims, (H, K, m)
    # the test networks and the shapes of XV
    assert {M.V_SHAPES[c.shape][:2] for c in M.V_CASES} == {(50, 9), (11, 2), (64, 4), (128, 2), (70, 5), (160, 20), (129, 17)}
    for s in M.V_SHAPES:
        assert {c.kind for c in M.V_CASES if c.shape == s} == set(M.V_KINDS), s
    assert any(c.kind == 'points' and c.N == 1 for c in M.V_CASES)
    for W, q, fam, kw, _ in M.V_SHAPES.values():
        assert KN.testnet_family(W, q) == fam and KN.testnet_kwidth(W, q) == kw, (W, q)


def test_inputs_and_cotangents_have_the_layouts_the_tables_name():
    X = M._place(M.paths(5, 3, 2, 1), 'float32', 'host', 'view', 'cpu')
    assert X.dtype == torch.float32 and not X.is_contiguous() and tuple(X.shape) == (5, 3, 3)
    assert torch.equal(X.contiguous(), M.paths(5, 3, 2, 1).float())
    g = M.cotangent('expand', (5, 3), 0, 'cpu')
    assert 0 in g.stride()[:2] and tuple(g.shape) == (5, 3, 1)
    g = M.cotangent('transposed', (5, 3), 0, 'cpu')
    assert not g.is_contiguous() and g.stride()[:2] == (1, 5) and float(g.std()) > 0
    g = M.cotangent('transposed', (2, 3, 5), 0, 'cpu')
    assert not g.is_contiguous() and tuple(g.shape) == (2, 3, 5, 1)
    assert M.cotangent('contiguous', (4,), 0, 'cpu').is_contiguous()


# ---- the stand-ins pass --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', M.U_CASES, ids=M.case_id)
def test_stand_in_passes_the_u_comparisons(c):
    with M.standin():
        M.run_u_case(c, 'cpu')


@pytest.mark.parametrize('c', M.V_CASES, ids=M.case_id)
def test_stand_in_passes_the_v_comparisons(c):
    with M.standin():
        M.run_v_case(c, 'cpu')


@pytest.mark.parametrize('boundary', [False, True])
@pytest.mark.parametrize('shape,solver,stepper,N', M.SLICE_CASES)
def test_stand_in_passes_the_single_slice_comparisons(shape, solver, stepper, N, boundary):
    with M.standin():
        M.run_slice_case(shape, solver, stepper, N, 'cpu', boundary)


# ---- planted defects: every comparison can fail --------------------------------------------------------------------------------
def _first(cases, **want):
    return next(c for c in cases if all(getattr(c, k) == v for k, v in want.items()) and c.N > 1)


@pytest.mark.parametrize('defect,run', [
    ('cot_transposed', lambda d: M.run_u_case(_first(M.U_CASES, cot='contiguous', shape='exact20'), 'cpu', d)),
    ('cot_transposed', lambda d: M.run_u_case(_first(M.U_CASES, cot='transposed', shape='tiled33'), 'cpu', d)),
    ('last_path_dropped', lambda d: M.run_u_case(_first(M.U_CASES, shape='c32', solver='midpoint'), 'cpu', d)),
    ('last_path_dropped', lambda d: M.run_v_case(_first(M.V_CASES, kind='points'), 'cpu', d)),
    ('last_time_dropped', lambda d: M.run_u_case(_first(M.U_CASES, shape='embed7', L=5), 'cpu', d)),
    ('last_time_dropped', lambda d: M.run_v_case(_first(M.V_CASES, kind='paths'), 'cpu', d)),
    ('zeros_for_none', lambda d: M.run_slice_case('exact20', 'midpoint', None, 17, 'cpu', False, d)),
    ('zeros_for_none', lambda d: M.run_slice_case('embed12', 'dopri5', 'vector', 15, 'cpu', True, d)),
    ('frozen_gets_grad', lambda d: M.run_u_case(_first(M.U_CASES, shape='c64'), 'cpu', d)),
    ('frozen_gets_grad', lambda d: M.run_v_case(_first(M.V_CASES, shape='w64'), 'cpu', d)),
    ('gx_channels_swapped', lambda d: M.run_u_case(_first(M.U_CASES, shape='generic48'), 'cpu', d)),
    ('gx_channels_swapped', lambda d: M.run_v_case(_first(M.V_CASES, shape='w128'), 'cpu', d)),
    ('wrong_ld', lambda d: M.run_u_case(_first(M.U_CASES, shape='embed7'), 'cpu', d)),
    ('wrong_ld', lambda d: M.run_v_case(_first(M.V_CASES, shape='embed11'), 'cpu', d)),
])
def test_a_planted_defect_fails_the_comparison(defect, run):
    assert defect in M.DEFECTS
    with M.standin():
        with pytest.raises(AssertionError):
            run(defect)


def test_every_defect_is_planted():
    import inspect
    src = inspect.getsource(sys.modules[__name__])
    for d in M.DEFECTS:
        assert "('%s'," % d in src, d


# ---- compat_loss: plain torch, pinned here ------------------------------------------------------------------------------------
def _oracle_nets(theta, phi, config, setup, funcs):
    from oracle import refspec as R
    return (lambda X: R.u_net_shaped(theta, config, setup, funcs, X)), (lambda XV: R.v_net(phi, config, XV).unsqueeze(2))


@pytest.mark.parametrize('case', ['ref_cone_groups', 'ref_hourglass_groups'])
def test_compat_loss_reproduces_the_list_domain_fixtures_on_oracle_networks(golden_dir, case):
    """the `loss` class over oracle networks (weights: refspec.init_parameters) in the reference's loop order: group 0 is the
    single-slice group at T0 with its [N, N] pairwise terms, group 1 a multi-slice one reached after Adam's first step; tolerances of
    test_sphere_domain_groups_against_reference_vectors.  Which parameters have no gradient and Adam's step counts: exactly."""
    from test_oracle_golden import _sphere_setup
    from oracle import refspec as R
    from xnode_wan_pde_solver_amd.compat_loss import loss
    from xnode_wan_pde_solver_amd.solver import func_eval
    z, params, config, setup, funcs, F, theta, phi, domain, triples = _sphere_setup(golden_dir, case)
    keys = [k for _, k in R.u_names(config['u_layers'])]
    theta = {k: torch.nn.Parameter(theta[k].clone()) for k in keys}
    opt = torch.optim.Adam([theta[k] for k in keys], lr=config['u_rate'])
    u_net, v_net = _oracle_nets(theta, phi, config, setup, funcs)
    fresh = lambda t: t.detach().clone().requires_grad_(True)       # noqa: E731
    assert triples[0][0].shape[1] == 1 and triples[1][0].shape[1] > 1
    opt.zero_grad()
    for step, (X, XV, BX) in enumerate(triples[:2]):
        tag = 'step%d' % step
        datau, datav, bdata = fresh(X), fresh(XV), fresh(BX)
        pv, pu = v_net(datav), u_net(datau)
        assert pu.dim() == (2 if step == 0 else 3)
        h, f, g, a, b, c = func_eval(datau.clone().detach(), bdata.clone().detach(), setup, pu, F.func_a, F.func_b, F.func_c, F.func_h,
                                     F.func_f, F.func_g)
        Lo = loss(config['alpha'], a, b, c, h, f, g, setup, domain, torch.device('cpu'))
        with torch.no_grad():
            np.testing.assert_allclose(float(Lo.init(pu)), float(z[tag + '/init']), rtol=1e-9)
            np.testing.assert_allclose(float(Lo.bdry(u_net, bdata)), float(z[tag + '/bdry']), rtol=1e-9)
        L = Lo.u(pu, pv, u_net, datau, datav, bdata)
        np.testing.assert_allclose(L.item(), float(z[tag + '/loss']), rtol=1e-5)
        assert float(datau.grad.abs().max()) == 0.0 and float(datav.grad.abs().max()) == 0.0      # (left zeroed by I, as documented)
        L.backward()
        has = np.concatenate([np.full(theta[k].numel(), theta[k].grad is not None) for k in keys])
        assert np.array_equal(has, z[tag + '/has_grad']), tag
        grad = np.concatenate([(theta[k].grad if theta[k].grad is not None else torch.zeros_like(theta[k])).numpy().reshape(-1) for k in keys])
        ref = z[tag + '/grad']
        np.testing.assert_allclose(grad, ref, rtol=1e-5, atol=1e-6 * float(np.abs(ref).max()))
        opt.step()
        steps = [int(opt.state[theta[k]]['step']) if theta[k] in opt.state else 0 for k in keys]
        assert steps == [int(s) for s in z[tag + '/adam_steps']], tag
        after = np.concatenate([theta[k].detach().numpy().reshape(-1) for k in keys])
        np.testing.assert_allclose(after, z[tag + '/after'], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize('L', [1, 4])
@pytest.mark.parametrize('N', [1, 6])
def test_compat_loss_I_is_the_oracle_weak_form_on_general_coefficients(N, L):
    """loss.I against refspec.weak_I_shaped with seeded general a_ij, b_i, c(u): the value and its gradients with respect to both
    networks' parameters at 1e-12, on a single-slice group ([N, 1] outputs: the pairwise forms) and on a multi-slice one"""
    from oracle import refspec as R
    from xnode_wan_pde_solver_amd.compat_loss import loss
    d = 3
    config, setup = M._cfg(20, 10, 3, W=12, q=2), M._setup(d)
    theta, phi = M._weights(config, d, 77)
    theta = {k: v.requires_grad_(True) for k, v in theta.items()}
    phi = {k: v.requires_grad_(True) for k, v in phi.items()}
    funcs = dict(h=M.smooth_h, g=M.smooth_g)
    domain = R.Ball('NSphere_TCone', 1.0, d, 0.0, 1.0)
    g_ = torch.Generator().manual_seed(78 + N + L)
    X0 = M.paths(N, L, d, 79) * 0.3
    X0[:, :, 0] = torch.linspace(0, 0.5, L)[:L].view(1, L) if L > 1 else 0.0
    a = torch.randn(d, d, N, L, dtype=F64, generator=g_)
    b = torch.randn(d, N, L, dtype=F64, generator=g_)
    f = torch.randn(N, L, dtype=F64, generator=g_)
    h = torch.randn(N, dtype=F64, generator=g_)
    kap = torch.randn(N, L, dtype=F64, generator=g_)
    out = []
    for which in ('compat', 'oracle'):
        X, XV = X0.clone().requires_grad_(True), (X0 * 0.9).clone().requires_grad_(True)
        u_s = R.u_net_shaped(theta, config, setup, funcs, X)
        v3 = R.v_net(phi, config, XV).unsqueeze(2)
        assert tuple(u_s.shape) == ((N, 1) if L == 1 else (N, L, 1))
        c_s = (kap if L == 1 else kap.unsqueeze(2)) * u_s ** 2            # a reaction term that is differentiated through
        if which == 'compat':
            Lo = loss(1.0, a, b, c_s, h, f, None, setup, domain, torch.device('cpu'))
            I = Lo.I(u_s, v3, X, XV)
            assert float(X.grad.abs().max()) == 0.0 and float(XV.grad.abs().max()) == 0.0
            for p in list(theta.values()) + list(phi.values()):         # (the helper backward passes' side effect, not compared here)
                p.grad = None
        else:
            w = domain.func_w(XV)
            du = torch.autograd.grad(u_s.sum(), X, retain_graph=True)[0]
            dphi = torch.autograd.grad((v3 * w.unsqueeze(2)).sum(), XV, retain_graph=True)[0]
            I = R.weak_I_shaped(setup, domain.V(), u_s, v3, w.detach(), du, dphi, h, f, a, b, c_s)
        keys = [k for k in M.U_ORDER] + M.V_ORDER
        gr = torch.autograd.grad(I, [theta[k] for k in M.U_ORDER] + [phi[k] for k in M.V_ORDER], allow_unused=True)
        out.append((I.detach(), dict(zip(keys, gr))))
    (Ic, gc), (Io, go) = out
    assert abs(float(Ic) - float(Io)) <= 1e-12 * abs(float(Io)), (float(Ic), float(Io))
    scale = max(float(g.abs().max()) for g in go.values() if g is not None)
    for k in go:
        assert (gc[k] is None) == (go[k] is None), k
        if go[k] is not None:
            assert float((gc[k] - go[k]).abs().max()) <= 1e-12 * scale, k
    if L == 1:
        assert all(go[k] is None for k in R.FIELD_KEYS)


def test_refusals_keep_their_messages_and_the_evaluation_path_carries_gradients():
    with M.standin():
        M.check_refusals('cpu')
        M.run_bound_pad_case('cpu')
