"""The merged generator sweep: XwOdeBwdJob.res_first_only == 3 (cotangent A + (2/I) B formed inside ONE interior sweep) and the
generator sub-step built on it (Engine._gen_front_merged, xw_substep_gen with XwSolverState.merged_sweep).

Kernel level, shapes N in {1, 5, 17, 33} x L in {2, 3}: a lone path, a ragged tile, a second tile with one live path; with L = 2
the first and the last time index fall into the same (only) step, with L = 3 there is a middle index that is neither.  Containers:
the headline (H, K, m) = (20, 10, 8) and the wide (64, 16); in addition one width of the generic path and one of the tiled family,
which form the cotangent through csrc/xw_generic_cot.h.

Tolerances are those of the tests this file leans on:
  kind 3 against the materialised array   1e-13 in test_gpu_kernels._close's metric -- what
      tests/test_gpu_kernels.py::test_ode_sweep_with_residual_cotangents asks of kind 2 against the stored ubarB
  linearity                                1e-11 relative to the largest entry -- tests/test_gpu_fullsize.py::
      test_stepper_sweeps_at_full_size's check of sweep(u1 + 2 u2) against sweep(u1) + 2 sweep(u2)
  engine against the oracle                tests/test_gpu_engine.py::_first_iteration itself, with the switch on and off
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

F64 = torch.float64
D = 3
SHAPES = [(N, L) for N in (1, 5, 17, 33) for L in (2, 3)]
VOL, NG, ALPHA, POLL, KAPPA, I_VAL = 3.7, 41.0, 5.0, 1.0, -0.8, 0.37


def _close(a, b, tol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(float(b.abs().max()), 1e-300)
    err = float((a - b).abs().max()) / scale
    print('%s: %.3e (scale %.3e)' % (what, err, scale))
    assert err < tol, '%s: max rel-to-scale error %.3e (scale %.3e)' % (what, err, scale)


class _Case:
    """one forward pass at (family, H, K, m, solver, N, L) and the operands of the generator's cotangents over it"""

    def __init__(self, family, H, K, m, solver, N, L, narrow=False):
        from xnode_wan_pde_solver_amd import kernels as KN
        self.KN, self.family, self.N, self.L, self.narrow = KN, family, N, L, narrow
        g = torch.Generator().manual_seed(1000 * N + 10 * L + H)
        dev = torch.device('cuda')
        self.M = (KN.method_id(solver), H, K, m)
        self.th = (0.3 * torch.randn(KN.theta_size(D, H, K), generator=g, dtype=F64)).to(dev)
        xT = (torch.rand(D, N, generator=g, dtype=F64) * 2 - 1).to(dev)
        t = torch.sort(torch.rand(L, generator=g, dtype=F64)).values
        t[0], t[-1] = 0.0, 1.0
        self.t = t.to(dev)
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64).to(dev)  # noqa: E731
        u, Y = torch.empty(L, N, dtype=F64, device=dev), torch.empty(L, H, N, dtype=F64, device=dev)
        self.job = dict(xT=xT, start=rnd(N), u=u, Y=Y)
        rows = KN.ode_act_rows(self.M[0], H, K, m) if family == 'fused' else 0
        if rows:
            self.job['act'] = torch.empty(L - 1, rows, KN.ode_act_cols(N), dtype=F64, device=dev)
        if family == 'tiled':
            KN.tiled_ode_fwd_multi([self.job], self.t, self.th, *self.M)
        else:
            KN.ode_fwd_multi([self.job], self.t, self.th, *self.M, narrow=narrow)
        self.has_store = bool(rows)
        self.u, self.h, self.v = u, rnd(N), rnd(L, N)
        self.w_n, self.w_ln = torch.rand(N, generator=g, dtype=F64).to(dev), torch.rand(L, N, generator=g, dtype=F64).to(dev)
        self.c, self.cp = rnd(L, N), rnd(L, N)
        self.scal = torch.zeros(16, dtype=F64, device=dev)
        self.scal[0] = I_VAL

    def res(self, kind, per_point, tab):
        """the residual dict of kind 1 (A), 2 (B) or 3 (merged) for kernels.ode_bwd_multi"""
        A = dict(ref=self.h, coef=2.0 * ALPHA / NG, base=POLL)
        if kind == 1:
            return dict(u=self.u, first_only=True, **A)
        B = dict(u=self.u, ref=self.v, coef=VOL / NG / self.L, base=VOL / NG,
                 weak=dict(w=self.w_ln if per_point else self.w_n, c=self.c if tab else None, cp=self.cp if tab else None,
                           ckappa=0.0 if tab else KAPPA))
        if kind == 3:
            B['merged'] = dict(scal=self.scal, **A)
        return B

    def stored(self, per_point, tab):
        """A + (2/I) B as an array: xw_gen_cotangents' merged form"""
        ubar = torch.empty(self.L, self.N, dtype=F64, device=self.u.device)
        self.KN.gen_cotangents(self.u, self.v, self.w_ln if per_point else self.w_n, self.h, VOL, NG, ALPHA, ubar, None,
                               c=self.c if tab else None, cp=self.cp if tab else None, ckappa=0.0 if tab else KAPPA,
                               pollution=POLL, scal=self.scal)
        return ubar

    def sweep(self, with_store=True, **cot):
        """the summed parameter gradient of one sweep with the cotangent `cot` (ubar=... or res=...)"""
        KN = self.KN
        j = dict(self.job, **cot)
        if not with_store:
            j['act'] = None
        if self.family == 'tiled':
            slab = torch.full((KN.lib.xw_tiled_ode_bwd_slabs(self.N), self.th.numel()), float('nan'), dtype=F64, device=self.u.device)
            KN.tiled_ode_bwd_multi([dict(j, gslab=slab)], self.t, self.th, *self.M, want_x=False, want_params=True)
        else:
            slab = torch.full((KN.ode_bwd_slabs(self.N), self.th.numel()), float('nan'), dtype=F64, device=self.u.device)
            KN.ode_bwd_multi([dict(j, gslab=slab)], self.t, self.th, *self.M, want_x=False, want_params=True,
                             narrow=self.narrow and with_store)
        assert torch.isfinite(slab).all()
        return KN.slab_sum(slab)


def _cases(family, H, K, m, solver):
    for N, L in SHAPES:
        yield _Case(family, H, K, m, solver, N, L)
        if family == 'fused' and (H, K) == (20, 10) and solver != 'rk4':      # narrow tiles: this container, from the store
            yield _Case(family, H, K, m, solver, N, L, narrow=True)


FAMILIES = [('fused', 20, 10, 8), ('fused', 64, 16, 8), ('generic', 48, 16, 3), ('tiled', 72, 24, 3)]


@pytest.mark.parametrize('solver', ['euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize('family,H,K,m', FAMILIES)
def test_merged_kind_against_the_materialised_cotangent(family, H, K, m, solver):
    """the sweep fed the array of xw_gen_cotangents(scal=...) against the sweep that forms A + (2/I) B itself (kind 3): c = kappa u
    with a weight per path and tabulated c, c' with a weight per point; 16-path and narrow tiles; from the store and recomputing.
    1e-13, the bound of test_gpu_kernels.test_ode_sweep_with_residual_cotangents for kind 2 against the stored ubarB."""
    for cs in _cases(family, H, K, m, solver):
        for per_point, tab in ((False, False), (True, True)):
            ubar = cs.stored(per_point, tab)
            for with_store in ([True, False] if cs.has_store and not cs.narrow else [cs.has_store]):
                want = cs.sweep(with_store, ubar=ubar)
                got = cs.sweep(with_store, res=cs.res(3, per_point, tab))
                _close(got, want, 1e-13, 'kind 3 against the array: %s (%d, %d) %s N %d L %d narrow %s store %s tab %s'
                       % (family, H, K, solver, cs.N, cs.L, cs.narrow, with_store, tab))


@pytest.mark.parametrize('solver', ['euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize('family,H,K,m', FAMILIES)
def test_merged_kind_is_the_sum_of_its_parts(family, H, K, m, solver):
    """slabs of kind 3 against slabs(kind 1) + s slabs(kind 2), s = 2 / I: 1e-11, the bound of the linearity check of
    test_gpu_fullsize.test_stepper_sweeps_at_full_size"""
    s = 2.0 / I_VAL
    for cs in _cases(family, H, K, m, solver):
        for per_point, tab in ((False, False), (True, True)):
            gA = cs.sweep(res=cs.res(1, per_point, tab))
            gB = cs.sweep(res=cs.res(2, per_point, tab))
            gM = cs.sweep(res=cs.res(3, per_point, tab))
            _close(gM, gA + s * gB, 1e-11, 'linearity: %s (%d, %d) %s N %d L %d narrow %s tab %s'
                   % (family, H, K, solver, cs.N, cs.L, cs.narrow, tab))


@pytest.mark.parametrize('family,H,K,m', FAMILIES)
def test_merged_kind_refuses_incomplete_jobs(family, H, K, m):
    """kind 3 without the scalar pointer, the weight, v or the initial penalty's reference: XW_E_ARG from every family's entry point,
    before anything is launched; the complete job runs.  (Every stepper family forms kind 3: the fused containers in
    csrc/xw_ode_core.h, the generic path, the tiled family and both dopri5 steppers through csrc/xw_generic_cot.h -- there is no
    family left to refuse the kind itself; an unknown kind, 4, is refused.)"""
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XwOdeBwdJob, lib
    cs = _Case(family, H, K, m, 'midpoint', 17, 3)
    p = lambda x: x.data_ptr()  # noqa: E731
    slab = torch.full(((17 + 15) // 16, cs.th.numel()), float('nan'), dtype=F64, device='cuda')   # (the complete job must write it)
    work = KN.tiled_ode_work(True, D, H, K, m, 2, slab.device) if family == 'tiled' else None

    def call(**drop):
        arr = (XwOdeBwdJob * 1)()
        a = arr[0]
        a.xT, a.start, a.Y, a.N, a.gslab = p(cs.job['xT']), p(cs.job['start']), p(cs.job['Y']), 17, p(slab)
        a.act = p(cs.job['act']) if cs.has_store else 0
        a.res_first_only, a.res_u, a.res_ref, a.res_w, a.res_w_per_point = 3, p(cs.u), p(cs.v), p(cs.w_n), 0
        a.res_coef, a.res_base, a.res_kappa2 = VOL / NG / 3, VOL / NG, 2.0 * KAPPA
        a.res_scal, a.res_refA, a.res_coefA, a.res_baseA = p(cs.scal), p(cs.h), 2.0 * ALPHA / NG, POLL
        for k, v in drop.items():
            setattr(a, k, v)
        if family == 'tiled':
            return lib.xw_tiled_ode_bwd_multi(arr, 1, p(cs.t), p(cs.th), 1, 3, D, H, K, m, 2, p(work), KN._stream())
        return lib.xw_ode_bwd_multi(arr, 1, p(cs.t), p(cs.th), 1, 3, D, H, K, m, 2, KN._stream())

    for field in ('res_scal', 'res_w', 'res_ref', 'res_refA', 'res_u'):
        assert call(**{field: 0}) == -2, field              # XW_E_ARG
    assert call(res_first_only=4) == -2
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(slab).all()


# ---- the engine ------------------------------------------------------------------------------------------------------------------
ORACLE_CASES = ['ref_tiny_midpoint', 'ref_min_d2_nt2_midpoint', 'ref_nr1_d3_midpoint', 'ref_nb1_d3_midpoint', 'ref_d20_small_midpoint']


@pytest.mark.parametrize('merged', [True, False])
@pytest.mark.parametrize('case', ORACLE_CASES)
def test_generator_substep_against_the_reference_vectors(golden_dir, case, merged):
    """tests/test_gpu_engine.py::_first_iteration -- u, v, nabla_x u, the penalties, loss_u, every parameter's gradient and the
    parameters after Adam of the first (and second) generator sub-step against the reference's record, at that test's tolerances --
    with the merged sweep on and off"""
    from test_gpu_engine import _first_iteration
    from xnode_wan_pde_solver_amd.options import EngineOptions
    G = _first_iteration(golden_dir, case, options=EngineOptions(merged_sweep=merged))
    assert bool(G.merged) == merged


def _solver(options=None, domain='Hypercube', **over):
    from test_gpu_engine import make_solver
    params = {'alpha': 1e4, 'u_layers': 8, 'u_hidden_dim': 20, 'u_hidden_hidden_dim': 10, 'v_layers': 9, 'v_hidden_dim': 50,
              'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'midpoint',
              'dim': 3, 'N_t': 3, 'N_r': 33, 'N_b': 17, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 1, 'domain': domain}
    params.update(over)
    return make_solver(params, 5, options=options)


def _three_cycles(variant, merged=True):
    from test_gpu_engine import first_sample
    from xnode_wan_pde_solver_amd.options import EngineOptions
    opts = dict(wide=dict(compact_tiles=0), compact=dict(compact_tiles=10 ** 6), skip_v=dict(reuse_test_net=True),
                eager=dict(use_graphs=False), one_stream=dict(use_graphs=False, use_streams=False), runner={})[variant]
    S = _solver(EngineOptions(merged_sweep=merged, **opts))
    eng = S.engine
    domain, pts = first_sample(S)
    G = eng.load_group(pts.interioru, pts.interiorv, pts.boundary, domain)
    assert (G.N, G.Nb, G.L) == (33, 17, 3)
    if variant == 'runner':
        G.persistent = False
        assert eng._runner_ok(G)
    out = []
    for _ in range(3):
        for kind in 'ggd':
            (eng.generator_step if kind == 'g' else eng.discriminator_step)(G)
            out += [eng.theta.data.clone(), eng.phi.data.clone(), eng.scal[4:6].clone(), eng.grad_u.clone()]
    if variant == 'skip_v':
        assert any('vcached' in k for k in G.graphs)                  # (the second g of a cycle reused v)
    if variant != 'runner':                                            # (the runner decides inside the C call)
        assert bool(G.merged) == merged
    assert all(bool(torch.isfinite(x).all()) for x in out)
    return out


def test_every_variant_of_the_merged_substep_gives_the_same_bits():
    """wide captured graph, compact schedule, reused test network, eager launches (with and without side streams) and the native
    runner xw_substep_gen: the same launches on the same arguments -- theta, phi, both losses and grad_u bit for bit after every
    sub-step of three g, g, d cycles at N = 33, N_b = 17, L = 3; and twice the same variant.  (Under the merged form `compact_tiles`
    is not consulted, so 'wide' against 'compact' only shows that the option does not leak into it; the comparisons that take
    different code are skip_v, eager, one_stream and the runner.)"""
    ref = _three_cycles('wide')
    for variant in ('wide', 'compact', 'skip_v', 'eager', 'one_stream', 'runner'):
        got = _three_cycles(variant)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), '%s differs from the wide graph at output %d' % (variant, i)


def test_groups_outside_the_merged_form_keep_their_bits():
    """a carried gradient (a sub-iteration over several groups) and a pairwise single-slice group must not take the merged form:
    with the switch on they compute what they compute with it off"""
    from test_gpu_engine import first_sample
    from src.dataset import Comb_loader
    from xnode_wan_pde_solver_amd.options import EngineOptions
    outs = []
    for merged in (True, False):
        S = _solver(EngineOptions(merged_sweep=merged))
        eng = S.engine
        domain, pts = first_sample(S)
        G = eng.load_group(pts.interioru, pts.interiorv, pts.boundary, domain)
        eng.begin_substep('u', True)
        eng.generator_step(G)
        eng.generator_step(G)
        assert not G.merged and eng.accum_u is not None
        outs.append([eng.theta.data.clone(), eng.grad_u.clone(), eng.scal.clone()])
        S = _solver(EngineOptions(merged_sweep=merged), domain='NSphere_TCone', dim=4, N_t=8, N_r=300, N_b=200, shape_param=1.0)
        eng = S.engine
        s = S.setup
        domain = S.domain(s['shape_param'], s['dim'], s['T0'], s['T'], s['N_t'])
        pts = Comb_loader(s['N_r'], s['N_b'], domain, S.device)
        G0 = eng.load_group(pts.interioru[0], pts.interiorv[0], pts.boundary[0], domain)
        assert G0.pair_i and G0.L == 1
        eng.generator_step(G0)
        assert not G0.__dict__.get('merged', False) and eng.accum_u is None
        outs[-1] += [eng.theta.data.clone(), eng.grad_u.clone(), eng.scal.clone()]
    for i, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a, b), 'output %d moved with the switch' % i
