"""Edge shapes of the wave-per-tile kernel families inside a guard-banded, poisoned arena (tests/guarded.py): the tiled stepper
(csrc/xw_tiled.hip: euler, midpoint, rk4, explicit_adams), dopri5 on it (csrc/xw_tdopri.hip), the tiled test network
(csrc/xw_disc_tiled.hip) and, under the same guards, the fused (64, 16) container, the narrow-tile sweeps and the test network's
MFMA containers (96 / 128, and the 50 / 64 kernels of the flagship workload over a covering selection of their own).

Every case
  * takes every operand -- inputs, outputs, slabs, and through guarded.Arena.workspaces the tiled families' workspaces -- from one
    Arena: outputs and workspaces start as a NaN pattern, inputs are followed by it, every view sits between guard bands;
  * after the launches calls Arena.check: no guard element changed, every output element written, every region the kernels leave
    alone by design (stated per case, from the kernels' code) still the pattern;
  * is compared with the oracle's autograd (oracle/refspec.py restated as tests/test_gpu_tiled_stepper._oracle does, with
    tests/adams_ref.py and tests/dopri5_ref.py), never with another kernel family, in the project's metric (_close: max error
    relative to the reference's scale) at the project's tolerances: 1e-12 on u / Y / v, 1e-11 on tangents, 1e-10 on gradients,
    parameter gradients per key and summed; dopri5 at tests/test_gpu_dopri5_tiled.py's 1e-9 / GRID_TOL, for the reasons given there
    (the one-path, one-unit fixture alone has a grid bound of its own, from the restatement's conditioning: _grid_tolerance).

The cases are a seeded covering selection, not a product: every listed value of every axis occurs at least once with every method
and with every cotangent form (the test network: every mode and every ngrad kind, and every width with every depth and with every point count).  The module
asserts its own coverage table when it is collected.

Regions pinned as untouched (from the code):
  tiled stepper / dopri5 sweep    gslab of a sweep without want_params (no memset, no slab pointer); gx and gs of a sweep without
                                  want_x
  tiled test network              the record's columns of the points past N L in its last 16-point tile (only valid points store);
                                  vt, gxv, gtv where not requested are not passed at all
  test-network MFMA containers    nothing: the record's padding columns ARE written (every lane of the ragged last tile stores a copy
                                  of the last valid point into a slot of its own, csrc/xw_disc_fwd.hip k_disc_fwd): all of it is checked
  fused containers                nothing: the activation store's padding columns ARE written (padding paths hold copies and have
                                  slots of their own, csrc/xw_ode_core.h act_store).  At (64, 16) every double row of the store is
                                  checked as written; at (20, 10) the partial 4-row block (K mod 4 = 2) leaves slots unused inside the
                                  record, so the narrow-tile cases check its guards only
                                  (this file's cases.  tests/test_gpu_stepper_inventory.py pins more, from act_store: the 16-path
                                  forward's full store has every double row written in all three containers, its x-only store the tanh
                                  rows written and the other double rows untouched; the narrow-tile forward's store stays guard-checked)

Tolerances at the widest / deepest corners: ORACLE_SPREAD below holds the float64 oracle's own rounding spread, measured on the CPU
(oracle_spread(): the case as written against the same case with hidden units permuted and the path order reversed --
mathematically identical, so the difference is rounding alone), in _close's metric.  Where a spread exceeds an eighth of the
project tolerance the case's tolerance is 8 x the spread (the kernel's MFMA accumulation is a third summation order); elsewhere the
project tolerance stands.  `python tests/test_gpu_edges.py` prints the table (CPU only).
"""
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import adams_ref as A  # noqa: E402
import guarded as G  # noqa: E402
from test_gpu_tiled_stepper import F64, U_ORDER, _close, _sample, _theta  # noqa: E402

pytestmark = pytest.mark.gpu

V_ORDER = ['Vin', 'Vin_b', 'Vh', 'Vh_b', 'Vo', 'Vo_b']
TOL_VALUE, TOL_TANGENT, TOL_GRAD = 1e-12, 1e-11, 1e-10
DEVICE = 'cuda'


# ---- the covering selection --------------------------------------------------------------------------------------------------------
def cover(axes, partners, pairs=(), fixed=None, seed=0, tries=300):
    """cases (dicts over `axes` and `partners`) such that every value of every axis occurs with every value of every partner, and
    every combination of the axis pairs in `pairs` occurs: greedy over seeded random candidates.  fixed(rnd, case): adjusts a
    candidate (dependent axes)."""
    rnd = random.Random(seed)
    need = set()
    for ax, vals in axes.items():
        for v in vals:
            for pa, pvals in partners.items():
                need.update((ax, v, pa, w) for w in pvals)
    for a, b in pairs:
        need.update((a, v, b, w) for v in axes[a] for w in axes[b])

    def hits(c):
        return {(ax, c[ax], pa, c[pa]) for ax in axes for pa in partners} | {(a, c[a], b, c[b]) for a, b in pairs}

    cases = []
    while need:
        best, gain = None, -1
        for _ in range(tries):
            c = {k: rnd.choice(list(v)) for k, v in list(axes.items()) + list(partners.items())}
            if fixed is not None:
                fixed(rnd, c)
            g_ = len(hits(c) & need)
            if g_ > gain:
                best, gain = c, g_
        assert gain > 0
        need -= hits(best)
        cases.append(best)
    return cases


def missing(cases, axes, partners, pairs=()):
    """the coverage table's holes: (axis, value, partner, value) combinations no case reaches"""
    seen = set()
    for c in cases:
        seen.update((ax, c[ax], pa, c[pa]) for ax in axes for pa in partners)
        seen.update((a, c[a], b, c[b]) for a, b in pairs)
    want = {(ax, v, pa, w) for ax, vals in axes.items() for v in vals for pa, pv in partners.items() for w in pv}
    want |= {(a, v, b, w) for a, b in pairs for v in axes[a] for w in axes[b]}
    return sorted(want - seen, key=repr)


D_MAX = 126                                         # the largest input dimension of the C ABI (csrc/xw_common.h: d + 2 <= 128 input rows)


def _check_d_max():
    """D_MAX is what the tiled family's ABI accepts and one more is refused (asked of the library when a case runs, not when the
    module is collected)"""
    from xnode_wan_pde_solver_amd._lib import lib
    assert lib.xw_tiled_ode_work(0, D_MAX, 1, 1, 1) > 0 and lib.xw_tiled_ode_work(0, D_MAX + 1, 1, 1, 1) < 0


# ---- the tiled stepper ------------------------------------------------------------------------------------------------------------
METHODS = ('euler', 'midpoint', 'rk4', 'explicit_adams')
FORMS = ('ubar', 'res', 'res_first', 'ones_x', 'x_only', 'params_only')
NAMED = ((1, 1, 1), (256, 1, 1), (1, 256, 3), (17, 17, 2), (255, 255, 2), (256, 256, 32))
STEPPER_AXES = {
    'N': (1, 2, 15, 16, 17, 31, 32, 33, 47),
    'H': (1, 3, 4, 15, 16, 17, 65, 255, 256),
    'K': (1, 3, 4, 15, 16, 17, 65, 255, 256),
    'm': (1, 2, 31, 32),
    'named': NAMED + (None,),                       # one of the named (H, K, m), or None: H, K, m drawn on their own
    'd': (1, 2, D_MAX),
    'L': (1, 2, 3, 12, 13),                         # L = 1: accepted by the ABI (L >= 1); 12 / 13: the Adams ring (11 slots) wraps
}
STEPPER_PARTNERS = {'method': METHODS, 'form': FORMS}


def _named(rnd, c):
    if c['named'] is not None:
        c['H'], c['K'], c['m'] = c['named']


def _stepper_cases():
    cases = cover(STEPPER_AXES, STEPPER_PARTNERS, fixed=_named, seed=13)
    for i, c in enumerate(cases):
        c['seed'] = 500 + i
    return cases


STEPPER_CASES = _stepper_cases()
assert not missing(STEPPER_CASES, STEPPER_AXES, STEPPER_PARTNERS), missing(STEPPER_CASES, STEPPER_AXES, STEPPER_PARTNERS)
assert 60 <= len(STEPPER_CASES) <= 100, len(STEPPER_CASES)


def _sid(c):
    return '%s-%s-N%d-H%dK%dm%d-d%d-L%d' % (c['method'], c['form'], c['N'], c['H'], c['K'], c['m'], c['d'], c['L'])


# The oracle's own rounding spread at the widest / deepest corners (oracle_spread below, float64, CPU): per case id
# (value spread: max over u, Y; gradient spread: max over gx, gs, every parameter's gradient and their sum).  Measured values are
# listed in profiles/r13_guarded_edges.md; a case is in this table when it is at (256, 256, 32) or at H = 1, K = 256.
ORACLE_SPREAD = {
    'midpoint-res-N17-H256K256m32-d1-L2': (1.01e-15, 2.29e-15),
    'euler-ubar-N17-H256K256m32-d1-L3': (1.36e-15, 2.13e-15),
    'explicit_adams-x_only-N2-H256K256m32-d1-L2': (2.23e-16, 4.55e-14),
    'rk4-ones_x-N15-H1K256m3-d1-L1': (0.0, 4.09e-16),
    'explicit_adams-params_only-N15-H256K256m32-d1-L2': (1.20e-15, 3.20e-15),
    'rk4-ones_x-N17-H256K256m32-d2-L13': (7.80e-16, 1.79e-15),
    'midpoint-res_first-N2-H1K256m3-d2-L1': (0.0, 0.0),
    'explicit_adams-res-N47-H1K256m3-d2-L13': (1.42e-14, 6.88e-15),
    'euler-x_only-N16-H1K256m3-d2-L13': (3.69e-16, 4.24e-15),
    'euler-params_only-N31-H1K256m3-d1-L3': (1.70e-15, 1.76e-15),
    'explicit_adams-ubar-N33-H1K256m3-d2-L2': (6.59e-16, 1.55e-15),
    'euler-res_first-N15-H256K256m32-d1-L13': (1.07e-15, 3.42e-15),
}                                                   # (every spread is below an eighth of its tolerance: the project's stand)


def _corner(c):
    return (c['H'], c['K'], c['m']) == (256, 256, 32) or (c['H'], c['K']) == (1, 256)


assert all(_sid(c) in ORACLE_SPREAD for c in STEPPER_CASES if _corner(c)) and all(
    any(_sid(c) == k for c in STEPPER_CASES) for k in ORACLE_SPREAD)


def _tolerances(c):
    """(values, gradients): the project's, or 8 x the oracle's measured spread where that exceeds an eighth of them"""
    sv, sg = ORACLE_SPREAD.get(_sid(c), (0.0, 0.0))
    return (8 * sv if sv > TOL_VALUE / 8 else TOL_VALUE), (8 * sg if sg > TOL_GRAD / 8 else TOL_GRAD)


def _lift(th, s):
    return torch.relu(torch.relu(s.view(-1, 1) @ th['IL0_w'].T + th['IL0_b']) @ th['IL2_w'].T + th['IL2_b']) @ th['IL4_w'].T + th['IL4_b']


def _oracle(theta, m, method, x, t, start):
    """the oracle's u [N, L] (attached), Y [L, H, N] and the leaves (x, start, the parameters in U_ORDER)"""
    from oracle import refspec as R
    th = {k: v.clone().requires_grad_(True) for k, v in theta.items()}
    x64 = x.clone().requires_grad_(True)
    s = start.clone().requires_grad_(True)
    f = lambda tt, y: R.field(th, m, x64, tt, y)                                # noqa: E731
    ys = A.explicit_adams(f, _lift(th, s), t) if method == 'explicit_adams' else R.odeint_fixed(f, _lift(th, s), t, method)
    u = (ys @ th['FL_w'].T + th['FL_b']).squeeze(2)
    return u, ys.detach().permute(1, 2, 0), [x64, s] + [th[k] for k in U_ORDER]


def _grads(u, leaves, cot):
    gs = torch.autograd.grad((u * cot).sum(), leaves, retain_graph=True, allow_unused=True)
    return [g if g is not None else torch.zeros_like(p) for g, p in zip(gs, leaves)]


def _check_params(flat, theta, want, tol, what):
    """the summed slab against the oracle's parameter gradients, per key and as a whole"""
    off = 0
    for k, g in zip(U_ORDER, want[2:]):
        n = theta[k].numel()
        _close(flat[off:off + n].view(theta[k].shape), g, tol, '%s grad %s' % (what, k))
        off += n
    assert off == flat.numel()
    _close(flat, torch.cat([g.reshape(-1) for g in want[2:]]), tol, what + ' summed parameter gradient')


def _cotangent(form, N, L, seed):
    """the host side of one cotangent form: (ubar [N, L] or None, res description or None)"""
    g = torch.Generator().manual_seed(seed)
    ubar = torch.randn(N, L, dtype=F64, generator=g)
    if form == 'res':
        return None, dict(ref=torch.randn(L, N, dtype=F64, generator=g), coef=0.7, base=0.2, first_only=False)
    if form == 'res_first':
        return None, dict(ref=torch.randn(N, dtype=F64, generator=g), coef=1.3, base=0.3, first_only=True)
    if form == 'ones_x':
        ubar[:, 1:] = 1.0                           # (x_cot_ones: the stored cotangent is 1 at every time index >= 1)
    return ubar, None


def _host_cot(ubar, res, u_dev):
    """the cotangent [N, L] a sweep job forms, from the device's own u [L, N] for the residual forms"""
    if res is None:
        return ubar
    if res['first_only']:
        cot = torch.full_like(u_dev, res['base'])
        cot[0] = res['base'] + res['coef'] * (u_dev[0] - res['ref'])
        return cot.t()
    return (res['base'] + res['coef'] * (u_dev - res['ref'])).t()


def _sweep_job(arena, fwd_job, form, ubar, res, d, N, P, slabs):
    """a sweep job in the arena for one cotangent form: (job, want_x, want_params, x_cot_ones, written, untouched)"""
    j = dict(fwd_job, gx=arena.out(d, N, name='gx'), gs=arena.out(N, name='gs'), gslab=arena.out(slabs, P, name='gslab'))
    if res is None:
        j['ubar'] = arena.inp(ubar.t(), name='ubar')
    else:
        j['res'] = dict(res, u=fwd_job['u'], ref=arena.inp(res['ref'], name='res.ref'))
    if form == 'x_only':
        return j, True, False, False, [j['gx'], j['gs']], [j['gslab']]
    if form == 'params_only':
        return j, False, True, False, [j['gslab']], [j['gx'], j['gs']]
    return j, True, True, form == 'ones_x', [j['gx'], j['gs'], j['gslab']], []


def _compare_sweep(KN, j, form, theta, u_ref, leaves, cot, tol, what):
    want = _grads(u_ref, leaves, cot)
    if form != 'params_only':
        wx = _grads(u_ref, leaves, torch.ones_like(cot)) if form == 'ones_x' else want
        _close(j['gx'].t(), wx[0], tol, what + ' gx')
        _close(j['gs'], wx[1], tol, what + ' gs')
    if form != 'x_only':
        _check_params(KN.slab_sum(j['gslab']).cpu(), theta, want, tol, what)


@pytest.mark.parametrize('c', STEPPER_CASES, ids=_sid)
def test_tiled_stepper_edges(c):
    from xnode_wan_pde_solver_amd import kernels as KN
    method, form, N, H, K, m, d, L = (c[k] for k in ('method', 'form', 'N', 'H', 'K', 'm', 'd', 'L'))
    assert KN.stepper_family(H, K, m, 'generic', KN.method_id(method)) in ('tiled', 'mfma')     # (a served shape)
    _check_d_max()
    tol_v, tol_g = _tolerances(c)
    theta, blob = _theta(H, K, m, d, c['seed'])
    x, t, start, _ = _sample(N, L, d, c['seed'] + 1000)
    ubar, res = _cotangent(form, N, L, c['seed'] + 2000)
    dev = torch.device(DEVICE)
    arena = G.Arena(dev)
    mid = KN.method_id(method)
    P = blob.numel()
    assert P == KN.theta_size(d, H, K)
    with arena.workspaces(KN):
        tc, bc = arena.inp(t, name='t'), arena.inp(blob, name='theta')
        fj = dict(xT=arena.inp(x.t(), name='xT'), start=arena.inp(start, name='start'), u=arena.out(L, N, name='u'),
                  Y=arena.out(L, H, N, name='Y'))
        KN.tiled_ode_fwd_multi([fj], tc, bc, mid, H, K, m)
        u_dev = fj['u'].cpu()
        j, want_x, want_params, ones, written, untouched = _sweep_job(arena, fj, form, ubar, res, d, N, P, KN.ode_bwd_slabs(N))
        KN.tiled_ode_bwd_multi([j], tc, bc, mid, H, K, m, want_x=want_x, want_params=want_params, x_cot_ones=ones)
    arena.check(written=[fj['u'], fj['Y']] + written, untouched=untouched)
    u_ref, Y_ref, leaves = _oracle(theta, m, method, x, t, start)
    _close(fj['u'].t(), u_ref.detach(), tol_v, 'u')
    _close(fj['Y'], Y_ref, tol_v, 'Y')
    _compare_sweep(KN, j, form, theta, u_ref, leaves, _host_cot(ubar, res, u_dev), tol_g, form)


# several jobs in one launch, a different cotangent form per job: the per-job workspace offsets of tiled_fwd / tiled_bwd
JOB_SIZES = (1, 16, 17, 33)
MULTI = [(method, H, K, m, d, L) for method in METHODS
         for H, K, m, d, L in ((17, 17, 2, 2, 13), (65, 15, 3, 1, 3), (256, 255, 1, 5, 12))]


@pytest.mark.parametrize('method,H,K,m,d,L', MULTI)
def test_tiled_stepper_several_jobs_in_one_launch(method, H, K, m, d, L):
    from xnode_wan_pde_solver_amd import kernels as KN
    theta, blob = _theta(H, K, m, d, 41)
    dev = torch.device(DEVICE)
    arena = G.Arena(dev)
    mid = KN.method_id(method)
    P = blob.numel()
    samples = [_sample(N, L, d, 42 + i) for i, N in enumerate(JOB_SIZES)]
    t = samples[0][1]
    with arena.workspaces(KN):
        tc, bc = arena.inp(t, name='t'), arena.inp(blob, name='theta')
        fjs = [dict(xT=arena.inp(x.t(), name='xT%d' % i), start=arena.inp(s, name='start%d' % i),
                    u=arena.out(L, x.shape[0], name='u%d' % i), Y=arena.out(L, H, x.shape[0], name='Y%d' % i))
               for i, (x, _, s, _) in enumerate(samples)]
        KN.tiled_ode_fwd_multi(fjs, tc, bc, mid, H, K, m)
        u_devs = [fj['u'].cpu() for fj in fjs]
        # launch A: residual / stored / residual / initial-value residual (the plain residual on the ragged jobs of 1 and 17
        # paths), x outputs and parameter gradients
        forms_a = ('res', 'ubar', 'res', 'res_first')
        cots_a = [_cotangent(f, N, L, 50 + i) for i, (f, N) in enumerate(zip(forms_a, JOB_SIZES))]
        ja = [_sweep_job(arena, fj, f, ub, rs, d, N, P, KN.ode_bwd_slabs(N)) for fj, f, (ub, rs), N in zip(fjs, forms_a, cots_a, JOB_SIZES)]
        KN.tiled_ode_bwd_multi([q[0] for q in ja], tc, bc, mid, H, K, m, want_x=True, want_params=True)
        # launch B: the all-ones x cotangent; the second and fourth job without x outputs, the fourth without a cotangent (ones)
        forms_b = ('res_first', 'ones_x', 'ones_x', None)
        cots_b = [(_cotangent(f, N, L, 60 + i) if f else (None, None)) for i, (f, N) in enumerate(zip(forms_b, JOB_SIZES))]
        cots_b[0][1].update(base=1.0)
        jb = []
        for i, (fj, (ub, rs), N) in enumerate(zip(fjs, cots_b, JOB_SIZES)):
            q = dict(fj, gslab=arena.out(KN.ode_bwd_slabs(N), P, name='gslabB%d' % i))
            if ub is not None:
                q['ubar'] = arena.inp(ub.t(), name='ubarB%d' % i)
            if rs is not None:
                q['res'] = dict(rs, u=fj['u'], ref=arena.inp(rs['ref'], name='res.refB%d' % i))
            if i in (0, 2):
                q.update(gx=arena.out(d, N, name='gxB%d' % i), gs=arena.out(N, name='gsB%d' % i))
            jb.append(q)
        KN.tiled_ode_bwd_multi(jb, tc, bc, mid, H, K, m, want_x=True, want_params=True, x_cot_ones=True)
    written = [v for fj in fjs for v in (fj['u'], fj['Y'])] + [v for q in ja for v in q[4]]
    written += [q[k] for q in jb for k in ('gx', 'gs', 'gslab') if k in q]
    arena.check(written=written)
    for i, (x, _, s, _) in enumerate(samples):
        u_ref, Y_ref, leaves = _oracle(theta, m, method, x, t, s)
        _close(fjs[i]['u'].t(), u_ref.detach(), TOL_VALUE, 'u job %d' % i)
        _close(fjs[i]['Y'], Y_ref, TOL_VALUE, 'Y job %d' % i)
        _compare_sweep(KN, ja[i][0], forms_a[i], theta, u_ref, leaves, _host_cot(*cots_a[i], u_devs[i]), TOL_GRAD, 'A job %d' % i)
        ub, rs = cots_b[i]
        cot = _host_cot(ub, rs, u_devs[i]) if (ub is not None or rs is not None) else torch.ones(JOB_SIZES[i], L, dtype=F64)
        want = _grads(u_ref, leaves, cot)
        _check_params(KN.slab_sum(jb[i]['gslab']).cpu(), theta, want, TOL_GRAD, 'B job %d' % i)
        if 'gx' in jb[i]:
            ones = _grads(u_ref, leaves, torch.ones_like(cot))
            _close(jb[i]['gx'].t(), ones[0], TOL_GRAD, 'B job %d gx (ones)' % i)
            _close(jb[i]['gs'], ones[1], TOL_GRAD, 'B job %d gs (ones)' % i)


# ---- dopri5 on the tiled stepper ---------------------------------------------------------------------------------------------------
# tanh-only fields (u_layers = 1: the step decisions are pinned exactly, tests/test_gpu_dopri5.py), at the network's own widths.
# (d, H, K, N, L, seed, form); every fixture's smallest |ratio - 1| of the restatement is asserted > 1e-9 before the comparison
DOPRI_CASES = [(1, 1, 1, 1, 2, 201, 'ubar'), (2, 17, 17, 15, 3, 202, 'res'), (3, 256, 1, 16, 4, 203, 'res_first'),
               (2, 1, 256, 17, 3, 204, 'ones_x'), (5, 255, 255, 33, 3, 205, 'x_only'), (1, 256, 256, 47, 4, 206, 'params_only'),
               (126, 65, 16, 2, 5, 207, 'ubar'), (4, 3, 4, 31, 13, 208, 'res'), (2, 16, 15, 32, 2, 209, 'ones_x'),
               (3, 15, 65, 17, 12, 210, 'res_first'), (2, 4, 3, 1, 3, 211, 'params_only'), (6, 17, 255, 15, 2, 212, 'x_only')]


# The restatement's own spread of the accepted grid per fixture seed (dopri5_grid_spread below: hidden units permuted, paths reversed;
# CPU, float64, the metric of GRID_TOL).  Section-4 rule: 8 x the spread where it exceeds an eighth of GRID_TOL (1.25e-10), else
# GRID_TOL.  Two fixtures are beyond it: K = 1 at H = 256 (seed 203: 1.8e-8) and (3, 4) with 11 attempts (seed 208: 5.6e-8).  The
# (1, 1, 1), one-path fixture (seed 201) has nothing to permute -- its measured spread is 0 -- and takes _grid_tolerance's bound.
DOPRI_GRID_SPREAD = {201: 0.0, 202: 3.53e-12, 203: 2.30e-9, 204: 8.52e-11, 205: 9.12e-13, 206: 2.23e-12, 207: 1.41e-11, 208: 6.95e-9,
                     209: 9.26e-13, 210: 3.27e-11, 211: 8.04e-11, 212: 5.53e-11}


def _dopri_grid_tol(d, H, K, N, L, seed, info=None):
    from test_gpu_dopri5 import GRID_TOL
    if (H, K, N) == (1, 1, 1):
        if info is None:
            from test_gpu_dopri5 import _case, _ref_Y
            cfg, theta, X, start = _case(d, H, K, 1, N, L, seed)
            _, info = _ref_Y(theta, cfg, X, start)
        return _grid_tolerance(info, GRID_TOL)
    s = DOPRI_GRID_SPREAD[seed]
    return 8 * s if s > GRID_TOL / 8 else GRID_TOL


@pytest.mark.parametrize('d,H,K,N,L,seed,form', DOPRI_CASES)
def test_tiled_dopri5_edges(d, H, K, N, L, seed, form):
    from test_gpu_dopri5 import GRID_TOL, _case, _grid_of, _ref_Y, _rel
    import dopri5_ref as D
    from xnode_wan_pde_solver_amd import kernels as KN
    m = 1
    cfg, theta, X, start = _case(d, H, K, m, N, L, seed)
    ys, info = _ref_Y(theta, cfg, X, start)
    assert info['gap'] > 1e-9, 'bad fixture: a step decision within %.1e of the threshold' % info['gap']
    u_ref = (ys @ theta['FL_w'].T + theta['FL_b']).squeeze(2)
    blob = torch.cat([theta[k].reshape(-1) for k in U_ORDER])
    ubar, res = _cotangent(form, N, L, seed + 7)
    dev = torch.device(DEVICE)
    arena = G.Arena(dev)
    P = blob.numel()
    assert P == KN.theta_size(d, H, K)
    with arena.workspaces(KN):
        tc, bc = arena.inp(X[0, :, 0].double(), name='t'), arena.inp(blob, name='theta')
        fj = dict(xT=arena.inp(X[:, 0, 1:].double().t(), name='xT'), start=arena.inp(start, name='start'), u=arena.out(L, N, name='u'),
                  Y=arena.out(L, H, N, name='Y'))
        rec, = KN.dopri5_fwd([fj], tc, bc, H, K, m, H, stepper='tiled')
        u_dev = fj['u'].cpu()
        j, want_x, want_params, ones, written, untouched = _sweep_job(arena, dict(fj, rec=rec), form, ubar, res, d, N, P,
                                                                      KN.ode_bwd_slabs(N))
        KN.dopri5_sweep([j], tc, bc, H, K, m, want_x=want_x, want_params=want_params, x_cot_ones=ones, stepper='tiled')
    arena.check(written=[fj['u'], fj['Y']] + written, untouched=untouched)
    print('dopri5 edge', (d, H, K, N, L, seed, form), 'device', (rec.n_att, rec.n_acc), 'ref', (info['n_att'], info['n_acc']), 'gap', info['gap'])
    assert (rec.n_att, rec.n_acc) == (info['n_att'], info['n_acc'])
    grid_tol = _dopri_grid_tol(d, H, K, N, L, seed, info)
    print('grid', _rel(rec.grid, _grid_of(info)), 'bound', grid_tol, 'cond', ['%.1e%s' % (c_, '' if free else ' (clamped)') for c_, free in info['cond']])
    assert _rel(rec.grid, _grid_of(info)) < grid_tol
    assert _rel(fj['u'].t(), u_ref) < 1e-9
    assert _rel(fj['Y'].permute(2, 0, 1), ys) < 1e-9
    # the sweep against autograd through the restatement on the device's accepted grid (step sizes as constants)
    th = {k: v.clone().requires_grad_(True) for k, v in theta.items()}
    x64 = X[:, 0, 1:].double().clone().requires_grad_(True)
    s = start.clone().requires_grad_(True)
    Xd = torch.cat((X[:, :, :1].double(), x64.view(N, 1, -1).expand(N, L, -1)), 2)
    u_r, _ = D.u_net(th, cfg, Xd, s, frozen=rec.steps)
    _compare_sweep_dopri(KN, j, form, theta, u_r, [x64, s] + [th[k] for k in U_ORDER], _host_cot(ubar, res, u_dev))


def _grid_tolerance(info, grid_tol):
    """the bound on the accepted grid's relative error for the ONE fixture with one path and one hidden unit, (d, H, K, N) =
    (1, 1, 1, 1), from the restatement alone; the other fixtures: _dopri_grid_tol.  GRID_TOL's reasoning (tests/test_gpu_dopri5.py)
    is that the error estimate is a sum of terms ~1e4 times larger than itself.  With one path and one unit nothing is averaged and
    the cancellation is far stronger: info['cond'] (tests/dopri5_ref.py) is, per attempt, sum |dt E_q k_q| / |sum dt E_q k_q| in the
    ratio's norm -- 8.6e9 at this fixture's second attempt (5e5 .. 3e6 at the wide fixtures).  There is no unit and no path to
    permute, so the oracle's spread cannot be measured by reordering; the bound is reasoned instead: each stage value k_q carries up
    to ~2 units of rounding (a dot product and a tanh) on either side of the comparison, so the two ratios differ by up to
    4 eps cond, the next step size (ratio^(-1/5), where the factor is not clamped) by a fifth of that, and the perturbations of
    successive steps add: 4 eps sum(cond) / 5 = 1.5e-6.  Measured on the device: 1.4e-7."""
    eps = 2.0 ** -52
    return max(grid_tol, 4 * eps * sum(c for c, free in info['cond'] if free) / 5)


def _compare_sweep_dopri(KN, j, form, theta, u_ref, leaves, cot):
    from test_gpu_dopri5 import _rel
    want = _grads(u_ref, leaves, cot)
    if form != 'params_only':
        wx = _grads(u_ref, leaves, torch.ones_like(cot)) if form == 'ones_x' else want
        assert _rel(j['gx'].t(), wx[0]) < 1e-9 and _rel(j['gs'], wx[1]) < 1e-9, form
    if form != 'x_only':
        flat, off = KN.slab_sum(j['gslab']).cpu(), 0
        for k, g in zip(U_ORDER, want[2:]):
            n = theta[k].numel()
            assert _rel(flat[off:off + n].view(theta[k].shape), g) < 1e-9, (form, k)
            off += n
        assert _rel(flat, torch.cat([g.reshape(-1) for g in want[2:]])) < 1e-9, form


# ---- the fused families under the same guards ----------------------------------------------------------------------------------------
def _fused_oracle(H, K, m, d, N, L, solver, seed):
    from oracle import refspec as R
    from test_gpu_kernels import _sample as ksample, _setup
    cfg = {'alpha': 1.0, 'u_layers': m, 'u_hidden_dim': H, 'u_hidden_hidden_dim': K, 'v_layers': 2, 'v_hidden_dim': 50,
           'n1': 1, 'n2': 1, 'u_rate': 0.01, 'v_rate': 0.01, 'min_steps': 5, 'adjoint': False, 'solver': solver}
    torch.manual_seed(seed)
    theta, _ = R.init_parameters(cfg, _setup(d, 2))
    for p in theta.values():
        if p.dim() == 1:
            p.copy_(0.3 * torch.randn_like(p))
    x, t, _ = ksample(N, L, d, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    start = torch.randn(N, dtype=F64, generator=g)
    ubar = torch.randn(N, L, dtype=F64, generator=g)
    u_ref, Y_ref, leaves = _oracle(theta, m, solver, x.double(), t.double(), start)
    blob = torch.cat([theta[k].reshape(-1) for k in U_ORDER])
    return theta, blob, x.double(), t.double(), start, ubar, u_ref, Y_ref, leaves


# (N, L, d, m, solver): the (64, 16) container, every case with and without the activation store (rk4 has none)
WIDE_CASES = [(1, 2, 1, 1, 'euler'), (15, 3, 2, 10, 'midpoint'), (16, 2, 20, 5, 'rk4'), (17, 5, 3, 2, 'euler'), (33, 3, 7, 10, 'rk4'),
              (47, 2, 4, 9, 'midpoint'), (2, 4, 2, 3, 'midpoint'), (31, 2, 20, 1, 'rk4')]


@pytest.mark.parametrize('N,L,d,m,solver', WIDE_CASES)
def test_wide_container_under_guards(N, L, d, m, solver):
    from xnode_wan_pde_solver_amd import kernels as KN
    H, K = 64, 16
    assert KN.stepper_family(H, K, m) == 'mfma'
    theta, blob, x, t, start, ubar, u_ref, Y_ref, leaves = _fused_oracle(H, K, m, d, N, L, solver, 700 + N)
    want = _grads(u_ref, leaves, ubar)
    mid = KN.method_id(solver)
    rows = KN.ode_act_rows(mid, H, K, m)
    P = blob.numel()
    for with_act in ([False, True] if rows else [False]):
        arena = G.Arena(torch.device(DEVICE))
        tc, bc = arena.inp(t, name='t'), arena.inp(blob, name='theta')
        job = dict(xT=arena.inp(x.t(), name='xT'), start=arena.inp(start, name='start'), u=arena.out(L, N, name='u'),
                   Y=arena.out(L, H, N, name='Y'))
        if with_act:
            job['act'] = arena.out(L - 1, rows, KN.ode_act_cols(N), name='act')
        KN.ode_fwd_multi([job], tc, bc, mid, H, K, m)
        ub = arena.inp(ubar.t(), name='ubar')
        jx = dict(job, ubar=ub, gx=arena.out(d, N, name='gx'), gs=arena.out(N, name='gs'))
        KN.ode_bwd_multi([jx], tc, bc, mid, H, K, m, want_x=True, want_params=False)
        jp = dict(job, ubar=ub, gx=arena.out(d, N, name='gx2'), gs=arena.out(N, name='gs2'),
                  gslab=arena.out(KN.ode_bwd_slabs(N), P, name='gslab'))
        KN.ode_bwd_multi([jp], tc, bc, mid, H, K, m, want_x=True, want_params=True)
        written = [job['u'], job['Y'], jx['gx'], jx['gs'], jp['gx'], jp['gs'], jp['gslab']]
        if with_act:
            # the store is [step][tile of 16 paths][rows][16]; K = 16 has no partial 4-row block, and the padding paths of the last
            # tile store copies into slots of their own (csrc/xw_ode_core.h act_store): every double row is written.  The last
            # 2 x words rows per stage hold the ReLU-mask words, which are not doubles (two words at depth 10): guard-checked only
            words = 2 if 4 * (m - 1) > 32 else 1
            stages = 1 if solver == 'euler' else 2
            rec = job['act'].view(L - 1, KN.ode_act_cols(N) // 16, rows, 16)
            written.append(rec[:, :, :rows - 2 * words * stages, :])
        arena.check(written=written)
        what = 'store %s' % with_act
        _close(job['u'].t(), u_ref.detach(), TOL_VALUE, 'u ' + what)
        _close(job['Y'], Y_ref, TOL_VALUE, 'Y ' + what)
        for q in (jx, jp):
            _close(q['gx'].t(), want[0], TOL_GRAD, 'gx ' + what)
            _close(q['gs'], want[1], TOL_GRAD, 'gs ' + what)
        _check_params(KN.slab_sum(jp['gslab']).cpu(), theta, want, TOL_GRAD, what)


# (H, K, m, N, L, d, solver): the narrow-tile forward and sweeps (four waves of 4 paths per 16-path tile) from their own store
NARROW_CASES = [(20, 10, 8, 1, 3, 1, 'euler'), (20, 10, 1, 15, 2, 2, 'midpoint'), (20, 10, 10, 17, 4, 5, 'midpoint'),
                (32, 12, 10, 1, 2, 3, 'midpoint'), (32, 12, 2, 15, 3, 70, 'euler'), (32, 12, 8, 17, 3, 4, 'euler')]


@pytest.mark.parametrize('H,K,m,N,L,d,solver', NARROW_CASES)
def test_narrow_tiles_under_guards(H, K, m, N, L, d, solver):
    from xnode_wan_pde_solver_amd import kernels as KN
    theta, blob, x, t, start, ubar, u_ref, Y_ref, leaves = _fused_oracle(H, K, m, d, N, L, solver, 800 + N)
    want = _grads(u_ref, leaves, ubar)
    mid = KN.method_id(solver)
    rows = KN.ode_act_rows(mid, H, K, m)
    P = blob.numel()
    arena = G.Arena(torch.device(DEVICE))
    tc, bc = arena.inp(t, name='t'), arena.inp(blob, name='theta')
    job = dict(xT=arena.inp(x.t(), name='xT'), start=arena.inp(start, name='start'), u=arena.out(L, N, name='u'),
               Y=arena.out(L, H, N, name='Y'), act=arena.out(L - 1, rows, KN.ode_act_cols(N), name='act'))
    KN.ode_fwd_multi([job], tc, bc, mid, H, K, m, narrow=True)
    ub = arena.inp(ubar.t(), name='ubar')
    jx = dict(job, ubar=ub, gx=arena.out(d, N, name='gx'), gs=arena.out(N, name='gs'))
    KN.ode_bwd_multi([jx], tc, bc, mid, H, K, m, want_x=True, want_params=False, narrow=True)
    jp = dict(job, ubar=ub, gx=arena.out(d, N, name='gx2'), gs=arena.out(N, name='gs2'),
              gslab=arena.out(KN.ode_bwd_slabs(N), P, name='gslab'))
    KN.ode_bwd_multi([jp], tc, bc, mid, H, K, m, want_x=True, want_params=True, narrow=True)
    arena.check(written=[job['u'], job['Y'], jx['gx'], jx['gs'], jp['gx'], jp['gs'], jp['gslab']])
    _close(job['u'].t(), u_ref.detach(), TOL_VALUE, 'u')
    _close(job['Y'], Y_ref, TOL_VALUE, 'Y')
    for q in (jx, jp):
        _close(q['gx'].t(), want[0], TOL_GRAD, 'gx')
        _close(q['gs'], want[1], TOL_GRAD, 'gs')
    _check_params(KN.slab_sum(jp['gslab']).cpu(), theta, want, TOL_GRAD, 'narrow')


# ---- the test network ------------------------------------------------------------------------------------------------------------
POINTS = {1: (1, 1), 15: (5, 3), 16: (8, 2), 17: (17, 1), 63: (21, 3), 64: (16, 4), 65: (13, 5)}    # N L points as (N, L) in path mode
TESTNET_WIDTHS, TESTNET_DEPTHS = (1, 15, 16, 17, 129, 255, 256), (0, 1, 17, 32)
TESTNET_AXES = {'Wq': tuple((W, q) for W in TESTNET_WIDTHS for q in TESTNET_DEPTHS), 'W': TESTNET_WIDTHS, 'q': TESTNET_DEPTHS,
                'P': tuple(POINTS), 'd': (1, 5, D_MAX)}
TESTNET_PARTNERS = {'mode': ('path', 'point'), 'ngrad': ('0', '1', 'N')}      # every (W, q) with every mode and every ngrad kind
TESTNET_PAIRS = (('W', 'P'), ('q', 'P'), ('W', 'd'), ('P', 'd'))


def _wq(rnd, c):
    c['W'], c['q'] = c['Wq']


TESTNET_CASES = cover(TESTNET_AXES, TESTNET_PARTNERS, TESTNET_PAIRS, fixed=_wq, seed=17)
assert not missing(TESTNET_CASES, TESTNET_AXES, TESTNET_PARTNERS, TESTNET_PAIRS)
assert 60 <= len(TESTNET_CASES) <= 100, len(TESTNET_CASES)


def _testnet_reference(W, q, d, mode, P_, seed):
    """phi, the device operands' host values and the oracle's v, input gradient and parameter gradient; P_: a key of POINTS"""
    N, L = POINTS[P_] if mode == 'path' else (P_, 1)
    return _testnet_reference_nl(W, q, d, mode, N, L, seed)


def _testnet_reference_nl(W, q, d, mode, N, L, seed):
    """_testnet_reference at N paths x L times (path mode) / N points (point mode, L = 1); shared with
    tests/test_gpu_testnet_inventory.py"""
    from test_gpu_tiled_testnet import _phi, _reference
    cfg, phi = _phi(d, W, q, seed)
    g = torch.Generator().manual_seed(seed + 1)
    if mode == 'path':
        x = torch.rand(N, d, generator=g, dtype=F64) * 2 - 1
        t, _ = torch.sort(torch.rand(L, generator=g, dtype=F64))
        X = torch.cat((t.view(1, L, 1).expand(N, L, 1), x.view(N, 1, d).expand(N, L, d)), 2).contiguous()
        vbar = torch.randn(N, L, dtype=F64, generator=g)
        tpp = None
    else:
        assert L == 1
        x = torch.rand(N, d, generator=g, dtype=F64) * 2 - 1
        tpp = torch.rand(N, generator=g, dtype=F64)
        t = None
        X = torch.cat((tpp.view(N, 1), x), 1)
        vbar = torch.randn(N, dtype=F64, generator=g)
    v_ref, gX, gphi = _reference(phi, cfg, X, vbar, q)
    return phi, x, t, tpp, vbar, N, L, v_ref, gX, gphi


def _run_testnet(W, q, d, mode, P_, ngrad_kind, family, seed, max_blocks, table=False):
    """P_: a key of POINTS, or (N, L) -- in point mode the N L points of it; table: the input layer through disc_xproj's table"""
    from xnode_wan_pde_solver_amd import kernels as KN
    if isinstance(P_, tuple):
        N_, L_ = P_ if mode == 'path' else (P_[0] * P_[1], 1)
        phi, x, t, tpp, vbar, N, L, v_ref, gX, gphi = _testnet_reference_nl(W, q, d, mode, N_, L_, seed)
    else:
        phi, x, t, tpp, vbar, N, L, v_ref, gX, gphi = _testnet_reference(W, q, d, mode, P_, seed)
    ngrad = {'0': 0, '1': 1, 'N': N}[ngrad_kind]
    arena = G.Arena(torch.device(DEVICE))
    xT = arena.inp(x.t(), name='xT')
    blob = arena.inp(torch.cat([phi[k].reshape(-1) for k in V_ORDER]), name='phi')
    tc = arena.inp(t, name='t') if t is not None else None
    tp = arena.inp(tpp, name='tpp') if tpp is not None else None
    v, vt = arena.out(L, N, name='v'), arena.out(L, N, name='vt')
    gxv = arena.out(d, ngrad, name='gxv') if ngrad else None
    gtv = arena.out(ngrad, name='gtv') if ngrad else None
    rows, cols = KN.disc_act_rows(W, q, family), KN.disc_act_cols(N * L)
    act = arena.out(rows, cols, name='act')
    if table:
        xp = arena.out(KN.disc_xproj_rows(W), N, name='xproj')
        KN.disc_xproj(xT, blob, W, out=xp)
        KN.disc_fwd(xT, tc, blob, W, q, v=v, vt=vt, gxv=gxv, gtv=gtv, ngrad=ngrad, max_blocks=max_blocks, act=act, xproj=xp, family=family)
    else:
        KN.disc_fwd(xT, tc, blob, W, q, tpp=tp, v=v, vt=vt, gxv=gxv, gtv=gtv, ngrad=ngrad, max_blocks=max_blocks, act=act, family=family)
    vb = arena.inp(vbar.t() if mode == 'path' else vbar.view(1, -1), name='vbar')
    slab = arena.out(KN.disc_bwd_slabs(N, L), blob.numel(), name='gslab')
    KN.disc_bwd(xT, tc, blob, vb, W, q, tpp=tp, gslab=slab, act=act, family=family)
    written = [v, vt, slab] + ([gxv, gtv] if ngrad else [])
    untouched = []
    if family == 'tiled':
        # the record is [tiles of 16 points][rows][16]: the valid points' columns are written, the last tile's other columns are not
        rec = act.view(cols // 16, rows, 16)
        point = (torch.arange(cols // 16).view(-1, 1, 1) * 16 + torch.arange(16).view(1, 1, 16)).expand(cols // 16, rows, 16)
        written.append((rec, point < N * L))
        untouched.append((rec, point >= N * L))
    else:
        # the MFMA containers: every lane of the ragged last tile stores into a slot of its own (k_disc_fwd: the record's stores are
        # not masked by the point's validity, and k_disc_rec reads those columns with a zero cotangent): all of it is written
        written.append(act)
    if table:
        written.append(xp)
    arena.check(written=written, untouched=untouched)
    if table:
        _close(xp[:W].t(), x @ phi['Vin'][:, 1:].t() + phi['Vin_b'], TOL_VALUE, 'x projection')
        assert float(xp[W:].abs().sum()) == 0.0, 'padding rows of the x projection'
    if mode == 'path':
        _close(v.t(), v_ref, TOL_VALUE, 'v')
        _close(vt.t(), gX[:, :, 0], TOL_TANGENT, 'dv/dt')
        if ngrad:
            _close(gxv.t(), gX[:ngrad, 0, 1:], TOL_TANGENT, 'nabla_x v at t0')
            _close(gtv, gX[:ngrad, 0, 0], TOL_TANGENT, 'dv/dt (reverse) at t0')
    else:
        _close(v[0], v_ref, TOL_VALUE, 'v')
        _close(vt[0], gX[:, 0], TOL_TANGENT, 'dv/dt')
        if ngrad:
            _close(gxv.t(), gX[:ngrad, 1:], TOL_TANGENT, 'nabla_x v')
            _close(gtv, gX[:ngrad, 0], TOL_TANGENT, 'dv/dt (reverse)')
    flat, off = KN.slab_sum(slab).cpu(), 0
    for k in V_ORDER:
        n = phi[k].numel()
        _close(flat[off:off + n], gphi[off:off + n], TOL_GRAD, 'phi gradient ' + k)
        off += n
    _close(flat, gphi, TOL_GRAD, 'phi gradient (record)')


def _tid(c):
    return 'W%d-q%d-P%d-d%d-%s-ngrad%s' % (c['W'], c['q'], c['P'], c['d'], c['mode'], c['ngrad'])


@pytest.mark.parametrize('c', TESTNET_CASES, ids=_tid)
def test_tiled_testnet_edges(c):
    """forward, tangent, fused input gradient, record and the reverse from the record; max_blocks = 1: one block of four waves
    takes every 8-point tile in turn (several rounds from 33 points on)"""
    from xnode_wan_pde_solver_amd import kernels as KN
    assert KN.testnet_family(c['W'], c['q']) in KN.TESTNET_FAMILIES          # (a served shape)
    _run_testnet(c['W'], c['q'], c['d'], c['mode'], c['P'], c['ngrad'], 'tiled', 900 + TESTNET_CASES.index(c), 1)


@pytest.mark.parametrize('P_', tuple(POINTS))
@pytest.mark.parametrize('W', [96, 128])
def test_wide_testnet_containers_under_guards(W, P_):
    i = tuple(POINTS).index(P_) + (W == 128)
    _run_testnet(W, (9, 1, 16, 4)[i % 4], (5, 1, 20)[i % 3], ('path', 'point')[i % 2], P_, ('N', '1', '0')[i % 3], 'mfma', 950 + i, 1 + i % 2)


# the containers the benchmark runs (W = 50) and the one above it (64): forward with the fused gradient, record, reverse from it
MFMA_POINTS = tuple(POINTS.values()) + ((64, 2), (128, 1))                    # (N, L); point mode: the N L points of it
MFMA_AXES = {'W': (50, 64), 'q': (0, 1, 9, 16), 'P': MFMA_POINTS, 'd': (1, 5, 24, 25, 52, 53, D_MAX)}
MFMA_PARTNERS = {'mode': ('path', 'point'), 'ngrad': ('0', '1', 'N'), 'max_blocks': (1, 0), 'table': (True, False)}
MFMA_PAIRS = (('W', 'P'), ('q', 'P'), ('P', 'd'))


def _no_table_in_point_mode(rnd, c):
    """the x-projection table exists per path: a point-mode candidate with a table gives up one of the two"""
    if c['table'] and c['mode'] == 'point':
        if rnd.random() < 0.5:
            c['mode'] = 'path'
        else:
            c['table'] = False


MFMA_CASES = cover(MFMA_AXES, MFMA_PARTNERS, MFMA_PAIRS, fixed=_no_table_in_point_mode, seed=23)
assert not missing(MFMA_CASES, MFMA_AXES, MFMA_PARTNERS, MFMA_PAIRS)
assert 40 <= len(MFMA_CASES) <= 80, len(MFMA_CASES)


def _mid(c):
    return 'W%d-q%d-P%dx%d-d%d-%s-ngrad%s-cap%d%s' % (c['W'], c['q'], c['P'][0], c['P'][1], c['d'], c['mode'], c['ngrad'], c['max_blocks'],
                                                      '-table' if c['table'] else '')


@pytest.mark.parametrize('c', MFMA_CASES, ids=_mid)
def test_testnet_containers_50_64_under_guards(c):
    """the kernels of the flagship workload at the edge shapes: the input layer entirely or in part from LDS (d = 24 | 25, 52 | 53),
    from the x-projection table, one block taking every tile (max_blocks = 1: tickets from 65 points on) against the default cap"""
    _run_testnet(c['W'], c['q'], c['d'], c['mode'], c['P'], c['ngrad'], 'mfma', 960 + MFMA_CASES.index(c), c['max_blocks'], c['table'])


# ---- the oracle's own rounding spread (CPU) ------------------------------------------------------------------------------------------
def _permuted(theta, d, H, K, seed):
    """theta with the hidden units of both widths permuted (the same network), and the two permutations"""
    gen = torch.Generator().manual_seed(seed)
    ph, pk = torch.randperm(H, generator=gen), torch.randperm(K, generator=gen)
    tp = dict(theta)
    tp['IL0_w'], tp['IL0_b'] = theta['IL0_w'][ph], theta['IL0_b'][ph]
    tp['IL2_w'], tp['IL2_b'] = theta['IL2_w'][ph][:, ph], theta['IL2_b'][ph]
    tp['IL4_w'], tp['IL4_b'] = theta['IL4_w'][ph][:, ph], theta['IL4_b'][ph]
    cols = torch.cat((torch.arange(d + 1), d + 1 + ph))
    tp['Win'], tp['Win_b'] = theta['Win'][pk][:, cols], theta['Win_b'][pk]
    tp['Wh'], tp['Wh_b'] = theta['Wh'][pk][:, pk], theta['Wh_b'][pk]
    tp['Wo'], tp['Wo_b'] = theta['Wo'][ph][:, pk], theta['Wo_b'][ph]
    tp['FL_w'] = theta['FL_w'][:, ph]
    return {k: v.contiguous() for k, v in tp.items()}, ph, pk


def _unpermuted(k, v, d, inv_h, inv_k):
    """parameter k's gradient v of a network permuted by _permuted, back in the original order of the hidden units"""
    if k in ('IL0_w', 'IL0_b', 'IL2_b', 'IL4_b', 'Wo_b'):
        return v[inv_h]
    if k in ('IL2_w', 'IL4_w'):
        return v[inv_h][:, inv_h]
    if k == 'Win':
        return v[inv_k][:, torch.cat((torch.arange(d + 1), d + 1 + inv_h))]
    if k in ('Win_b', 'Wh_b'):
        return v[inv_k]
    if k == 'Wh':
        return v[inv_k][:, inv_k]
    if k == 'Wo':
        return v[inv_h][:, inv_k]
    if k == 'FL_w':
        return v[:, inv_h]
    return v


def dopri5_grid_spread(d, H, K, N, L, seed):
    """the restatement's own spread of the accepted grid for one dopri5 fixture (GRID_TOL's metric): as written against hidden units
    permuted and paths reversed; None if the two runs do not take the same attempts"""
    from test_gpu_dopri5 import _case, _grid_of, _ref_Y, _rel
    cfg, theta, X, start = _case(d, H, K, 1, N, L, seed)
    _, info = _ref_Y(theta, cfg, X, start)
    tp, _, _ = _permuted(theta, d, H, K, seed + 3000)
    rev = torch.arange(N - 1, -1, -1)
    _, info2 = _ref_Y(tp, cfg, X[rev].contiguous(), start[rev].contiguous())
    if (info['n_att'], info['n_acc']) != (info2['n_att'], info2['n_acc']):
        return None
    return _rel(_grid_of(info2), _grid_of(info))


def oracle_spread(c):
    """(value spread, gradient spread) of one stepper case in _close's metric: the oracle as written against the oracle with the
    hidden units of both widths permuted and the paths in reverse order (the same mathematics in another summation order)"""
    method, form, N, H, K, m, d, L = (c[k] for k in ('method', 'form', 'N', 'H', 'K', 'm', 'd', 'L'))
    theta, _ = _theta(H, K, m, d, c['seed'])
    x, t, start, _ = _sample(N, L, d, c['seed'] + 1000)
    ubar, res = _cotangent(form, N, L, c['seed'] + 2000)
    u, Y, leaves = _oracle(theta, m, method, x, t, start)
    cot = _host_cot(ubar, res, u.detach().t())
    g = _grads(u, leaves, cot)
    tp, ph, pk = _permuted(theta, d, H, K, c['seed'] + 3000)
    rev = torch.arange(N - 1, -1, -1)
    u2, Y2, leaves2 = _oracle(tp, m, method, x[rev].contiguous(), t, start[rev].contiguous())
    g2 = _grads(u2, leaves2, cot[rev].contiguous())
    inv_h, inv_k = torch.argsort(ph), torch.argsort(pk)

    def rel(a, b):
        return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)

    sv = max(rel(u2.detach()[rev], u.detach()), rel(Y2[:, inv_h][:, :, rev], Y))
    pairs = [(g2[0][rev], g[0]), (g2[1][rev], g[1])] + [(_unpermuted(k, a, d, inv_h, inv_k), b) for k, a, b in zip(U_ORDER, g2[2:], g[2:])]
    pairs.append((torch.cat([_unpermuted(k, a, d, inv_h, inv_k).reshape(-1) for k, a in zip(U_ORDER, g2[2:])]), torch.cat([b.reshape(-1) for b in g[2:]])))
    return sv, max(rel(a, b) for a, b in pairs)


if __name__ == '__main__':
    print('cases: tiled stepper %d (+ %d launches of several jobs), dopri5 %d, wide container %d, narrow tiles %d, tiled test '
          'network %d, 96 / 128 containers %d' % (len(STEPPER_CASES), len(MULTI), len(DOPRI_CASES), len(WIDE_CASES), len(NARROW_CASES),
                                                 len(TESTNET_CASES), 2 * len(POINTS)))
    print('| case | value spread | gradient spread | tolerance (values, gradients) |')
    for c_ in STEPPER_CASES:
        if _corner(c_):
            sv_, sg_ = oracle_spread(c_)
            print('| %s | %.2e | %.2e | %s |' % (_sid(c_), sv_, sg_, (8 * sv_ if sv_ > TOL_VALUE / 8 else TOL_VALUE,
                                                                     8 * sg_ if sg_ > TOL_GRAD / 8 else TOL_GRAD)))
    print('| dopri5 fixture (d, H, K, N, L, seed) | grid spread | grid tolerance |')
    for f_ in DOPRI_CASES:
        print('| %s | %.2e | %.2e |' % (f_[:6], dopri5_grid_spread(*f_[:6]), _dopri_grid_tol(*f_[:6])))
