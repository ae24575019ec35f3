"""The reference side of tests/test_gpu_weak.py -- TEST INFRASTRUCTURE ONLY (imported like tests/adams_ref.py; runs on the CPU).

The kernels of csrc/xw_weak.hip (k_weak_partials with grid_sum, k_bdry, k_gen_cots, k_disc_cot, k_losses, k_pair_fold, k_adam) take
time-major [L, N] operands and pre-digested pieces (the gradient contraction's factors, a factorised pairwise form).  This module
maps those operands onto the ORACLE's own functions (oracle/refspec.py: weak_I, weak_I_shaped, interior_loss, init_loss, bdry_loss,
adam_update, adam_update_sparse) in the oracle's shapes, evaluates them in float64 on the CPU and takes every cotangent by autograd.
The kernels' closed formulas are not typed out here.

    dphi[:, :, 0] = w vt + v wt         dphi[:, 0, 1:] = (w0 gxv + v[0] gwx0T)^T
    du[:, 0, 1:]  = (gx + gs ghT)^T     du = 0 at l > 0
    in-kernel contraction: a = identity, b = 0;   the s3x route: general a[d,d,N,L], b[d,N,L] (s3x itself comes from
    kernels.weak_contract_general on the device);   pairwise groups: weak_I_shaped on [N,1] / [N,1,1] shapes (the [N,N] broadcast
    is the oracle's);   a shard of a larger batch: n_glob;   s3_scale: the oracle's a, b, c, f times s3_scale / (the form's own factor).

Exact sums.  Every reduced scalar comes with the exact sum (math.fsum) of the terms that were added and with sum_abs, the sum of
their absolute values.  For I the terms are the oracle's own: I is linear in each of h, f, dphi[:, :, 0], a, b and c (as a table), so
its terms are X dI/dX per element of those operands (autograd through the oracle), and the u v term of s1 is v dI/dv of the oracle
with every other operand zero.

The case tables of the GPU module live here (the host tests walk the same cases); their coverage is asserted on import.
"""
import functools
import math
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F64 = torch.float64
TOL_SUM = 1e-13                 # reduced scalars: |got - exact| <= TOL_SUM * sum_abs
TOL_REF = 1e-14                 # the float64 oracle against the exact sum of the same terms (a tenth of TOL_SUM)
TOL_LOSS = 1e-11                # loss values (relative), the project's
TOL_ELEM = 1e-13                # elementwise outputs and Adam, _close's metric
MIN_I = 1e-2                    # finalised cases: |I| >= MIN_I * sum_abs, so that log I^2 is well conditioned
VOL, KAPPA, ALPHA = 2.5, 0.7, 1e3

# ---- the weak-form cases ---------------------------------------------------------------------------------------------------------------
NONPAIR = ((1, 1, 1), (5, 3, 7), (37, 7, 5), (64, 6, 6), (1030, 2, 3), (4099, 33, 4), (8195, 33, 4))
PAIR = ((1, 1, 1), (37, 1, 5), (1100, 1, 3))
SMALL_POINTS = 4096             # shapes of at most this many points also run under reduce_threads=256, reduce_blocks=3
REGIMES = ('L>d', 'L=d', 'L<d', 'pair')
AXES = {'weight': ('path', 'point'), 'wt': (False, True), 'c': ('kappa', 'table'), 'grad': ('inline', 's3x'),
        'href': (False, True), 'bdry': ('none', 'pb1', 'pbNL', 'pbGT', 'launch'), 'final': ('none', 'kernel', 'split'),
        'pollution': (1.0, 0.25), 's3': ('1', 'N')}
# shapes of a regime: the first ones are handed out once each, every further case of the regime takes the last (a small one)
REGIME_SHAPES = {'L>d': ((4099, 33, 4), (8195, 33, 4), (37, 7, 5)), 'L=d': ((1, 1, 1), (64, 6, 6)),
                 'L<d': ((1030, 2, 3), (5, 3, 7)), 'pair': ((1, 1, 1), (1100, 1, 3), (37, 1, 5))}


def regime(shape, pair):
    N, L, d = shape
    return 'pair' if pair else ('L>d' if L > d else 'L=d' if L == d else 'L<d')


def _wanted(axes, regimes):
    """(a reference of the initial penalty of its own, href, and an s3_scale other than 1 only exist in the pairwise form:
    kernels.weak_partials(pair=dict(href, s3_scale)))"""
    return {(ax, v, r) for ax, vals in axes.items() for v in vals for r in regimes
            if not (r != 'pair' and ((ax == 'href' and v) or (ax == 's3' and v == 'N')))}


def _cover(axes, regimes, seed=7, tries=200):
    """dicts over `axes` + 'regime' such that every value of every axis occurs with every regime (greedy, seeded)"""
    rnd = random.Random(seed)
    need = _wanted(axes, regimes)
    cases = []
    while need:
        best, gain = None, -1
        for _ in range(tries):
            c = {k: rnd.choice(v) for k, v in axes.items()}
            c['regime'] = rnd.choice(regimes)
            c['href'] = c['href'] and c['regime'] == 'pair'
            c['s3'] = c['s3'] if c['regime'] == 'pair' else '1'
            g = len({(ax, c[ax], c['regime']) for ax in axes} & need)
            if g > gain:
                best, gain = c, g
        need -= {(ax, best[ax], best['regime']) for ax in axes}
        cases.append(best)
    return cases


def missing(cases):
    seen = {(ax, c[ax], c['regime']) for c in cases for ax in AXES}
    return sorted(_wanted(AXES, REGIMES) - seen, key=repr)


def _weak_cases():
    cases = _cover(AXES, REGIMES)
    for r in REGIMES:
        mine = [c for c in cases if c['regime'] == r]
        for shape in REGIME_SHAPES[r][:-1]:
            # (one path cannot be split into two launches; the two large shapes are there for the launch shape of the WHOLE batch)
            c = next(c for c in mine if 'shape' not in c and not ((shape[0] == 1 or shape[0] * shape[1] > 128 * 1024) and c['final'] == 'split'))
            c['shape'] = shape
        for c in mine:
            c.setdefault('shape', REGIME_SHAPES[r][-1])
    for i, c in enumerate(cases):
        c['pair'] = c['regime'] == 'pair'
        c['seed'] = 4100 + i
        assert regime(c['shape'], c['pair']) == c['regime']
    return cases


def wid(c):
    return '%s%dx%dx%d-w%s%s-c%s-%s%s-b%s-%s-p%g-s%s' % ('pair' if c['pair'] else 'N', c['shape'][0], c['shape'][1], c['shape'][2],
                                                         c['weight'], '+wt' if c['wt'] else '', c['c'], c['grad'],
                                                         '-href' if c['href'] else '', c['bdry'], c['final'], c['pollution'], c['s3'])


WEAK_CASES = _weak_cases()
assert not missing(WEAK_CASES), missing(WEAK_CASES)
assert {(c['shape'], c['pair']) for c in WEAK_CASES} == {(s, False) for s in NONPAIR} | {(s, True) for s in PAIR}
assert len({wid(c) for c in WEAK_CASES}) == len(WEAK_CASES) and 20 <= len(WEAK_CASES) <= 40, len(WEAK_CASES)
SMALL_CASES = [c for c in WEAK_CASES if c['shape'][0] * c['shape'][1] <= SMALL_POINTS]
assert {regime(c['shape'], c['pair']) for c in SMALL_CASES} == set(REGIMES)

# The float64 oracle's own spread for a case that needs more than the tolerances above: {case id: spread} (rule of
# tests/test_gpu_edges.py: measured on the CPU, the case's tolerance is 8 x the spread; tests/test_weak_ref_host.py re-checks every
# entry).  No case needs it: every reference-vs-exact gap is below TOL_REF (profiles/r18_weak_kernels.md).
ORACLE_SPREAD = {}


def boundary_shape(c):
    """(Lb, Nb) of the boundary sample, or None.  Lb != L wherever the point count allows it."""
    N, L, _ = c['shape']
    P = N * L
    if c['bdry'] == 'none':
        return None
    if c['bdry'] == 'pb1':
        return (1, 1)
    if c['bdry'] == 'pbNL':
        return (1, P)
    if c['bdry'] == 'pbGT':
        Lb = 2 if L != 2 else 3
        return (Lb, P // Lb + 1)
    return (3, 300) if L != 3 else (2, 450)                                      # a launch of xw_bdry_partials of its own


def shards(c):
    """the path ranges of the launches: the whole batch, or two unequal parts that accumulate into one scal"""
    N = c['shape'][0]
    if c['final'] != 'split':
        return [(0, N)]
    n1 = max(1, (2 * N) // 3)
    return [(0, n1), (n1, N)]


# ---- the operands, in the kernels' layout ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = BY_ID[cid]
    (N, L, d), pair = c['shape'], c['pair']
    g = torch.Generator().manual_seed(c['seed'])
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)                      # noqa: E731
    pos = lambda *s: 0.5 + torch.rand(*s, generator=g, dtype=F64)                # noqa: E731
    # values with a common sign where a sum of them is a FACTOR (pairwise groups) and a mean well away from zero elsewhere, so that
    # I does not cancel to nothing against sum_abs (finalised cases need |I| >= MIN_I sum_abs); the d/dt and gradient terms change sign
    one = pos if pair else (lambda *s: 1.0 + 0.3 * rn(*s))
    o = dict(u=one(L, N), v=one(L, N), vt=pos(L, N) if pair else rn(L, N), h=rn(N), q=pos(L, N))
    o['f_nat'] = one(L, N)
    o['w'] = pos(L, N) if c['weight'] == 'point' else pos(N)
    o['wt'] = (pos(L, N) if pair else rn(L, N)) if c['wt'] else None
    o['w0'] = (o['w'][0] if c['weight'] == 'point' else o['w']).clone()
    for k in ('gx', 'ghT', 'gxv', 'gwx0T'):
        o[k] = rn(d, N)
    o['gs'] = rn(N)
    o['a0'] = (torch.eye(d, dtype=F64).view(d, d, 1) + 0.3 * rn(d, d, N)).contiguous() if c['grad'] == 's3x' else None
    # (the pairwise factorisation has no b term: sum_mn b_m phi_n du_m does not reduce to N sum_n, include/xnwan.h)
    o['b0'] = 0.3 * rn(d, N) if c['grad'] == 's3x' and not pair else None
    if c['href']:
        assert pair
        o['href'] = torch.full((N,), float(o['h'].mean()), dtype=F64)           # href := mean h
    else:
        o['href'] = None
    # the pairwise mean of src/loss.py:79 splits into mean_n (u_n - mean h)^2 + var h: the second part arrives as init_off
    o['init_off'] = float(o['h'].var(unbiased=False)) if (pair and c['href']) else 0.37
    o['bdry_off'] = 0.0 if c['bdry'] == 'none' else 0.21
    bs = boundary_shape(c)
    o['ub'], o['gb'] = (rn(*bs), rn(*bs)) if bs else (None, None)
    o['s3_scale'] = 1.0 if c['s3'] == '1' else float(N)
    o['f'] = torch.full((L, N), float(o['f_nat'].mean()), dtype=F64) if pair else o['f_nat']     # pairwise: f := mean f
    if c['c'] == 'table':
        o['c'] = torch.sin(o['u']) * o['q']
        o['cp'] = torch.cos(o['u']) * o['q']
    else:
        o['c'] = o['cp'] = None
    return o


def inputs(c):
    return _inputs(wid(c))


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------------
def _fsum(t):
    v = t.detach().reshape(-1).tolist()
    return math.fsum(v), math.fsum(abs(x) for x in v)


class Sum:
    """a reduced scalar: the float64 oracle's value, the exact sum of its terms and the sum of their absolute values"""

    def __init__(self, value, terms):
        self.value = float(value)
        parts = [_fsum(t) for t in terms]
        self.exact = math.fsum(p[0] for p in parts)        # (exact up to one rounding per operand group)
        self.sum_abs = math.fsum(p[1] for p in parts)

    def gap(self):
        return abs(self.value - self.exact) / max(self.sum_abs, 1e-300)


def _oracle_I(c, o, factor, u, v, c_leaf=None, zero_rest=False, no_dt=False):
    """I of the case through the oracle, from leaves u, v [N, L].  factor: what the oracle's a, b, c, f are multiplied with.
    c_leaf: c as a detached table (a leaf) instead of the function of u.  Returns I and the linear operands as leaves."""
    from oracle import refspec as R
    (N, L, d), pair = c['shape'], c['pair']
    setup = {'dim': d}
    T = lambda x: x.t().contiguous()                                             # noqa: E731
    w = T(o['w']) if c['weight'] == 'point' else o['w'].view(N, 1).expand(N, L).contiguous()
    z = 0.0 if zero_rest else 1.0
    dphit = w * T(o['vt'])
    if o['wt'] is not None:
        dphit = dphit + v.detach() * T(o['wt'])
    dphit = (z * (0.0 if no_dt else 1.0) * dphit).detach().requires_grad_(True)
    dphix = T(o['w0'] * o['gxv'] + o['v'][0] * o['gwx0T'])                       # [N, d]
    dux = z * T(o['gx'] + o['gs'] * o['ghT'])
    pad = torch.zeros(N, L - 1, d, dtype=F64)
    dphi = torch.cat((dphit.unsqueeze(2), torch.cat((dphix.unsqueeze(1), pad), 1)), 2)
    du = torch.cat((torch.zeros(N, L, 1, dtype=F64), torch.cat((dux.unsqueeze(1), pad), 1)), 2)
    a0 = o['a0'] if o['a0'] is not None else torch.eye(d, dtype=F64).view(d, d, 1).expand(d, d, N)
    a0 = (factor * a0).contiguous().requires_grad_(True)
    b0 = (factor * (o['b0'] if o['b0'] is not None else torch.zeros(d, N, dtype=F64))).requires_grad_(True)
    a = torch.cat((a0.unsqueeze(3), torch.zeros(d, d, N, L - 1, dtype=F64)), 3)  # (l > 0 multiplies du = 0)
    b = torch.cat((b0.unsqueeze(2), torch.zeros(d, N, L - 1, dtype=F64)), 2)
    h = (z * o['h']).requires_grad_(True)
    f = (z * factor * T(o['f_nat'])).requires_grad_(True)
    if c_leaf is not None:
        cu = c_leaf
    elif c['c'] == 'table':
        cu = factor * torch.sin(u) * T(o['q'])                                   # c = sin(u) q(x): cp is its derivative
    else:
        cu = factor * KAPPA * u
    if zero_rest:
        cu = 0.0 * cu
    tot = 0.0
    for lo, hi in ([(0, N)] if pair else shards(c)):                             # the oracle's n_glob form, shard by shard
        s = slice(lo, hi)
        if pair:
            tot = R.weak_I_shaped(setup, VOL, u, v.unsqueeze(2), w, du, dphi, h, f, a, b, cu)
        else:
            tot = tot + R.weak_I(setup, VOL, u[s], v[s], w[s], du[s], dphi[s], h[s], f[s], a[:, :, s], b[:, s], cu[s], n_glob=N)
    return tot, dict(h=h, f=f, dphit=dphit, a0=a0, b0=b0)


def _c_value(c, o, factor, u):
    T = lambda x: x.t().contiguous()                                             # noqa: E731
    return (factor * torch.sin(u) * T(o['q']) if c['c'] == 'table' else factor * KAPPA * u).detach()


def _I_terms(c, o, factor, no_dt=False):
    """(I, its terms): X dI/dX over the operands I is linear in, and the u v term of s1 from the oracle with the rest zero"""
    u, v = o['u'].t().contiguous(), o['v'].t().contiguous()
    cl = _c_value(c, o, factor, u).requires_grad_(True)
    I, lin = _oracle_I(c, o, factor, u, v, c_leaf=cl, no_dt=no_dt)
    ops = list(lin.values()) + [cl]
    gr = torch.autograd.grad(I, ops, allow_unused=True)
    terms = [x.detach() * g for x, g in zip(ops, gr) if g is not None]
    vl = v.clone().requires_grad_(True)
    I0, _ = _oracle_I(c, o, factor, u, vl, zero_rest=True)
    terms.append(v * torch.autograd.grad(I0, vl)[0])
    return float(I.detach()), terms


@functools.lru_cache(maxsize=None)
def _reference(cid):
    from oracle import refspec as R
    c = BY_ID[cid]
    o = inputs(c)
    (N, L, d), pair = c['shape'], c['pair']
    factor = o['s3_scale'] / (float(N) if pair else 1.0)
    r = {}
    I, terms = _I_terms(c, o, factor)
    r['I'] = Sum(I, terms)
    uo, vo = o['u'].t().contiguous(), o['v'].t().contiguous()
    hr = o['href'] if o['href'] is not None else o['h']
    r['S'] = Sum(torch.sum(vo ** 2), [vo ** 2])                                  # the sum inside R.interior_loss
    r['sse_init'] = Sum(R.init_loss(uo, hr) * N, [(uo[:, 0] - hr) ** 2])
    if o['ub'] is not None:
        r['sse_bdry'] = Sum(R.bdry_loss(o['ub'], o['gb']) * o['ub'].numel(), [(o['ub'] - o['gb']) ** 2])
    if pair:
        # the two factors of the pairwise d(phi)/dt term as the launch leaves them before the fold, and I without that term
        I1, t1 = _I_terms(c, o, factor, no_dt=True)
        r['I_unfolded'] = Sum(I1, t1)
        w = o['w'] if c['weight'] == 'point' else o['w'].view(1, N)
        dphit = w * o['vt'] + (o['v'] * o['wt'] if o['wt'] is not None else 0.0)
        r['sum_u'] = Sum(torch.sum(o['u']), [o['u']])
        r['sum_dphit'] = Sum(torch.sum(dphit), [dphit])
    # ---- loss values, combined as src/loss.py:93,96 ----
    u = uo.clone().requires_grad_(True)
    v = vo.clone().requires_grad_(True)
    Iu, _ = _oracle_I(c, o, factor, u, v)
    int_ = R.interior_loss(VOL, Iu, v.unsqueeze(2) if pair else v)
    if pair and c['href']:
        init_ = torch.mean((u[:, 0] - o['h'].unsqueeze(1)) ** 2)                 # all pairs, as R.group_forward writes it
    else:
        init_ = R.init_loss(u, hr) + o['init_off']
    bdry_ = (R.bdry_loss(o['ub'], o['gb']) if o['ub'] is not None else 0.0) + o['bdry_off']
    r['loss_u'] = float((int_ + ALPHA * (init_ + bdry_)).detach())
    r['loss_v'] = float(-int_.detach())
    r['int'] = float(int_.detach())
    # ---- cotangents, all by autograd ----
    wv = o['w'].t() if c['weight'] == 'point' else o['w'].view(N, 1)
    pol = c['pollution']
    r['vbar'] = torch.autograd.grad(pol * torch.sum(v * wv) - int_, v, retain_graph=True)[0].t().contiguous()
    if not pair:
        # k_gen_cots has no s3_scale: its I is the one with a, b, c, f as they are
        u1 = uo.clone().requires_grad_(True)
        I1, _ = _oracle_I(c, o, 1.0, u1, vo)
        r['I_gen'] = float(I1.detach())
        init1 = R.init_loss(u1, o['h'])
        r['ubarB'] = torch.autograd.grad(I1, u1, retain_graph=True)[0].t().contiguous()
        r['ubarA'] = torch.autograd.grad(pol * torch.sum(u1) + ALPHA * init1, u1, retain_graph=True)[0].t().contiguous()
        r['merged'] = torch.autograd.grad(pol * torch.sum(u1) + ALPHA * init1 + torch.log(I1 ** 2), u1)[0].t().contiguous()
    if c['bdry'] == 'launch':
        ub = o['ub'].clone().requires_grad_(True)
        r['ubar_b'] = torch.autograd.grad(ALPHA * R.bdry_loss(ub, o['gb']), ub)[0]
    return r


def reference(c):
    return _reference(wid(c))


BY_ID = {wid(c): c for c in WEAK_CASES}


# ---- the comparisons -------------------------------------------------------------------------------------------------------------------------
def check_sum(what, got, ref, tol=TOL_SUM):
    """a reduced scalar against the exact sum, relative to sum_abs"""
    got = float(got)
    err = abs(got - ref.exact)
    print('%s: got %.17g exact %.17g |diff| / sum_abs %.2e (bound %.0e)' % (what, got, ref.exact, err / max(ref.sum_abs, 1e-300), tol))
    assert math.isfinite(got) and err <= tol * ref.sum_abs, '%s: %.17g against %.17g, %.3e x sum_abs (%.3e)' % (
        what, got, ref.exact, err / max(ref.sum_abs, 1e-300), ref.sum_abs)


def check_loss(what, got, want, tol=TOL_LOSS):
    got = float(got)
    err = abs(got - want) / abs(want)
    print('%s: got %.17g want %.17g rel %.2e' % (what, got, want, err))
    assert math.isfinite(got) and err <= tol, '%s: %.17g against %.17g (rel %.3e)' % (what, got, want, err)


def close(a, b, tol, what):
    """the project's metric (tests/test_gpu_kernels._close): max error relative to the reference's scale"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.numel() == 0:
        return
    scale = max(float(b.abs().max()), 1e-300)
    err = float((a - b).abs().max()) / scale
    assert err < tol, '%s: max rel-to-scale error %.3e (scale %.3e)' % (what, err, scale)       # (NaN fails: not < tol)


def well_conditioned(c):
    """finalised cases: |I| >= MIN_I sum_abs (asserted on the reference side)"""
    r = reference(c)['I']
    return abs(r.exact) >= MIN_I * r.sum_abs


def check_weak_scal(c, scal, stage):
    """scal[0..8] of a case against the reference.  stage: 'sums' (after the launches, not finalised, not folded), 'final'"""
    r = reference(c)
    what = wid(c) + ' '
    if stage == 'sums' and c['pair']:
        check_sum(what + 'I before the fold', scal[0], r['I_unfolded'])
        check_sum(what + 'sum u', scal[7], r['sum_u'])
        check_sum(what + 'sum dphi/dt', scal[8], r['sum_dphit'])
    else:
        check_sum(what + 'I', scal[0], r['I'])
    check_sum(what + 'sum v^2', scal[1], r['S'])
    check_sum(what + 'SSE init', scal[2], r['sse_init'])
    if 'sse_bdry' in r:
        check_sum(what + 'SSE bdry', scal[3], r['sse_bdry'])
    if stage == 'final':
        assert well_conditioned(c)
        check_loss(what + 'loss_u', scal[4], r['loss_u'])
        check_loss(what + 'loss_v', scal[5], r['loss_v'])
        check_loss(what + 'int', scal[6], r['int'])
        if c['pair']:
            assert float(scal[7]) == 0.0 and float(scal[8]) == 0.0, 'the fold leaves scal[7], scal[8] at zero'


# ---- Adam ------------------------------------------------------------------------------------------------------------------------------------
ADAM_AXES = {'P': (1, 15, 16, 17, 1651), 'nA': (0, 1, 63, 64, 65, 130), 'nB': (0, 5, 70), 'extras': (False, True),
             'scal': (False, True), 'gsum': ('none', 'own', 'alias'), 'bump': (True, False, -1), 'lag': ('empty', 'all', '3-21')}
# a hand-made covering selection: every listed value of every axis occurs (asserted below); (3, 21) needs P > 21; the aliased
# gsum_out needs the extras
ADAM_CASES = [dict(zip(('P', 'nA', 'nB', 'extras', 'scal', 'gsum', 'bump', 'lag'), row)) for row in (
    (1, 0, 0, True, False, 'alias', True, 'all'),
    (1, 1, 5, False, True, 'none', -1, 'empty'),
    (15, 63, 70, True, True, 'own', False, 'all'),
    (16, 64, 0, False, False, 'own', True, 'empty'),
    (16, 130, 5, True, True, 'alias', -1, 'all'),
    (17, 65, 5, True, False, 'none', False, 'empty'),
    (17, 0, 70, False, True, 'own', True, 'all'),
    (1651, 130, 70, True, True, 'alias', False, '3-21'),
    (1651, 37, 5, True, True, 'none', True, '3-21'),
    (1651, 64, 0, False, False, 'own', -1, '3-21'),
    (1651, 1, 5, True, True, 'own', True, 'empty'),
)]
ADAM_AXES['nA'] += (37,)                     # (tests/test_gpu_kernels.test_adam_matches_torch_formula's slab counts, kept)
assert all({c[k] for c in ADAM_CASES} == set(v) for k, v in ADAM_AXES.items()), [k for k, v in ADAM_AXES.items() if {c[k] for c in ADAM_CASES} != set(v)]
SKIPS = (True, True, False, False)           # the four-update sequence: skip, skip, update, update (where there is a lagged range)
LR = 0.015


def aid(c):
    return 'P%d-nA%d-nB%d%s%s-gsum_%s-bump%s-lag_%s' % (c['P'], c['nA'], c['nB'], '-extras' if c['extras'] else '',
                                                       '-scal' if c['scal'] else '', c['gsum'], c['bump'], c['lag'])


def lag_range(c):
    return {'empty': (0, 0), 'all': (0, c['P']), '3-21': (3, 21)}[c['lag']]


@functools.lru_cache(maxsize=None)
def _adam_reference(cid):
    """per update: the operands, the summed gradient and param, m, v after it -- through R.adam_update_sparse over the segments
    [0, lo), [lo, hi), [hi, P) (gradient None on the lagged segment of a skipped update), R.adam_update where there is no lag"""
    from oracle import refspec as R
    c = ADAM_BY_ID[cid]
    P, (lo, hi) = c['P'], lag_range(c)
    g = torch.Generator().manual_seed(900 + ADAM_CASES.index(c))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)                      # noqa: E731
    p0 = rn(P)
    segs = [(k, a, b) for k, a, b in (('a', 0, lo), ('b', lo, hi), ('c', hi, P)) if b > a]
    p = {k: p0[a:b].clone() for k, a, b in segs} if hi > lo else {'p': p0.clone()}
    state, ups = {}, []
    for it, skip in enumerate(SKIPS):
        skip = skip and hi > lo
        ops = dict(A=rn(c['nA'], P) if c['nA'] else None, B=rn(c['nB'], P) if c['nB'] else None,
                   eA=rn(P) if c['extras'] else None, eB=rn(P) if c['extras'] else None, I=0.7 + it, skip=skip)
        grad = torch.zeros(P, dtype=F64)
        for x in (ops['eA'], ops['A'].sum(0) if ops['A'] is not None else None):
            grad = grad + x if x is not None else grad
        gb = torch.zeros(P, dtype=F64)
        for x in (ops['eB'], ops['B'].sum(0) if ops['B'] is not None else None):
            gb = gb + x if x is not None else gb
        grad = grad + (2.0 / ops['I'] if c['scal'] else 1.0) * gb
        if hi > lo:
            p = R.adam_update_sparse(p, {k: (None if (k == 'b' and skip) else grad[a:b]) for k, a, b in segs}, state, LR)
            cat = lambda pre: torch.cat([state.get(pre + k, torch.zeros(b - a, dtype=F64)) for k, a, b in segs])   # noqa: E731
            ups.append(dict(ops, g=grad, param=torch.cat([p[k] for k, a, b in segs]).clone(), m=cat('m_').clone(), v=cat('v_').clone()))
        else:
            p = R.adam_update(p, {'p': grad}, state, LR)
            ups.append(dict(ops, g=grad, param=p['p'].clone(), m=state['m_p'].clone(), v=state['v_p'].clone()))
    return dict(p0=p0, updates=ups, step=len(SKIPS), lag=sum(1 for s in SKIPS if s and hi > lo))


def adam_reference(c):
    return _adam_reference(aid(c))


ADAM_BY_ID = {aid(c): c for c in ADAM_CASES}
assert len(ADAM_BY_ID) == len(ADAM_CASES)


def check_adam(c, it, param, m, v, gsum=None, before=None):
    """param, m, v (and the summed gradient) after update `it`, per segment; before = (param, m, v) ahead of a skipped update: its
    lagged range must hold the same bits"""
    r = adam_reference(c)['updates'][it]
    lo, hi = lag_range(c)
    what = '%s update %d ' % (aid(c), it)
    for name, a, b in (('head', 0, lo), ('lagged', lo, hi), ('tail', hi, c['P'])):
        for k, got in (('param', param), ('m', m), ('v', v)):
            close(got[a:b], r[k][a:b], TOL_ELEM, what + k + ' ' + name)
    if gsum is not None:
        close(gsum, r['g'], TOL_ELEM, what + 'summed gradient')
    if r['skip']:
        for k, got, old in zip(('param', 'm', 'v'), (param, m, v), before):
            assert torch.equal(got[lo:hi].cpu().view(torch.int64), old[lo:hi].cpu().view(torch.int64)), what + k + ': the lagged range changed under skip'
