"""The two stepper families on the vector ALU -- the generic stepper (csrc/xw_generic.hip: kg_ode_fwd, kg_ode_bwd) and the vector
dopri5 stepper (csrc/xw_dopri.hip: kd_init1, kd_init2, kd_attempt, kd_sweep, each as <32> and as <64>) -- inside a guard-banded,
poisoned arena (tests/guarded.py), at the edges of their launch geometry (64 lanes per block, one gradient slab per 16 paths), in
every sweep mode and cotangent form, at the deepest and narrowest networks.  The case tables and what they cover: tests/vector_inventory.py.

Every case
  * takes every operand from one Arena: inputs, u, Y, gx, gs, the slabs, the operands of the residual cotangents and, through
    guarded.Arena.dopri5_records, the dopri5 record (rec_y, rec_t, rec_h, fbuf, work; every generation of a record that grows).
    Outputs start as the NaN pattern;
  * after the launches calls Arena.check once: no guard changed, every output element written, every region below still the pattern;
  * is compared with the oracle's autograd, never with another kernel family: oracle/refspec.py as tests/test_gpu_edges._oracle
    restates it (generic stepper), tests/dopri5_ref.py (dopri5: the step decisions exactly on the tanh-only fixtures, every other
    field and every sweep on the device's own accepted grid, frozen=rec.steps); parameter gradients per key at the network's own
    widths, from kernels.slab_sum;
  * runs every dopri5 forward twice: u, Y, the grid and (n_att, n_acc) are equal to the bit;
  * with several jobs in a call, runs every job alone as well: every output is equal to the bit.

Regions pinned as untouched (from the code):
  both sweeps         gslab without want_params (mode bit 1 clear: no memset, `slab` is null in every lane); gx and gs without want_x
                      (the stores sit behind `want_x &&`)
  dopri5 record       rec_y[n_acc + 1:], rec_t[n_acc + 1:], rec_h[n_acc:] after a forward.  kd_attempt writes its candidate to slot
                      n_acc + 1 whether or not it is accepted; the controller ends a job only after an ACCEPTED step (or with an
                      error status, which raises), so the last slot written is n_acc and a rejected candidate's slot is at most
                      n_acc, overwritten by the accepted step.  rec_t / rec_h are written by ctl_attempt on acceptance only.  The
                      surplus launches of the last chunk return at `c[C_DONE] != 0.0` before any store.
                      fbuf[1] (the f buffer of odd parity) where no attempt ran at all (t[L - 1] does not lie past t[0]: the
                      controller starts done).  A record that was replaced by grow() keeps its guards
  behind the slabs    the slab behind a job's last one (no 16-lane group past N owns one) is part of the case's memory and holds
                      -0.0, which adding zeros would turn into +0.0: checked bit for bit after every sweep
  written, not left   Y rows of the padding units of an embedded network (Hn < H): every row h < H is stored and those are exactly 0;
                      work (two partial sums per 64-path block: kd_init1 stores both of every block)
  not in the arena    the controller rows (torch.zeros in kernels.dopri5_fwd) and their page-locked mirror

Tolerances: the project's.  Generic stepper 1e-12 on u / Y and 1e-10 on every gradient in _close's metric (tests/test_gpu_kernels.py);
at the widest / deepest corners -- the (64, 16) width, u_layers = 32 -- the rule of tests/test_gpu_edges.py: ORACLE_SPREAD holds the
float64 oracle's own rounding spread (oracle_spread(): hidden units permuted, path order reversed; CPU), and where it exceeds an
eighth of the project tolerance the case's tolerance is 8 x the spread; `python tests/test_gpu_vector_paths.py` prints the table (CPU
only).  dopri5: 1e-9 and GRID_TOL of tests/test_gpu_dopri5.py for the reasons given there; a one-path fixture's grid bound is
test_gpu_edges._grid_tolerance, from the restatement's conditioning.  The two copies of the sweeps' l = 0 tail against each other:
TAIL_TOL, reasoned below.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dopri5_ref as D  # noqa: E402
import guarded as G  # noqa: E402
import test_gpu_edges as E  # noqa: E402
import vector_inventory as VI  # noqa: E402
from test_gpu_tiled_stepper import F64, U_ORDER, _close, _sample, _theta  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_VALUE, TOL_GRAD = 1e-12, 1e-10
DOPRI_TOL = 1e-9
DEVICE = 'cuda'
FLAGS = {'x': (True, False, False), 'params': (False, True, False), 'both': (True, True, False), 'both_ones': (True, True, True)}
# kg_ode_bwd's and kd_sweep's copies of the l = 0 tail are the same float64 expressions on the same inputs; what may differ between
# two compilations of them is which products the compiler contracts into a following add -- one rounding per term.  Every output is
# a sum of at most H = 64 such terms (per lift layer; the slab entries add 16 paths on top), so the two results differ by at most a
# few H eps relative to the output's scale: 4 x 64 x 2^-52
TAIL_TOL = 4 * 64 * 2.0 ** -52


# ---- cotangents --------------------------------------------------------------------------------------------------------------------
def _cot_host(form, ones, N, L, seed, u):
    """one cotangent form on the host: (the job's fields as host tensors, the cotangent [N, L] the sweep forms from them).  u: the
    forward's u [L, N] (the residual forms read it).  ones: the launch is x_cot_ones, whose contract is a cotangent of 1 at every
    time index >= 1 -- stored as such, or made so through the form's own operands (res: the residual vanishes there, base = 1;
    weak: v = 1 / (coef d(c u)/du w) there, base = 0), so that every form runs in that mode with an l = 0 value of its own"""
    g = torch.Generator().manual_seed(seed)
    if form == 'ubar':
        ubar = torch.randn(N, L, dtype=F64, generator=g)
        if ones:
            ubar[:, 1:] = 1.0
        return dict(ubar=ubar.t().contiguous()), ubar
    ref = torch.randn(L, N, dtype=F64, generator=g)
    if form == 'res':
        coef, base = 0.7, 1.0 if ones else 0.2
        if ones:
            ref[1:] = u[1:]
        return dict(res=dict(ref=ref, coef=coef, base=base, first_only=False)), (base + coef * (u - ref)).t().contiguous()
    if form == 'res_first':
        coef, base = 1.3, 1.0 if ones else 0.3
        cot = torch.full_like(u, base)
        cot[0] = base + coef * (u[0] - ref[0])
        return dict(res=dict(ref=ref[0].contiguous(), coef=coef, base=base, first_only=True)), cot.t().contiguous()
    assert form == 'weak'
    coef, base = 0.4, 0.0 if ones else 0.2
    per_point = seed % 2 == 1                               # the weight per point [L, N] or per path [N]
    w = torch.rand((L, N) if per_point else (N,), dtype=F64, generator=g) + 0.5
    if seed % 3 == 0:                                       # c and c' as tables, else c(u) = ckappa u^2
        tc, tcp = torch.randn(L, N, dtype=F64, generator=g), torch.randn(L, N, dtype=F64, generator=g)
        weak, dcu = dict(w=w, c=tc, cp=tcp), tc + u * tcp
    else:
        weak, dcu = dict(w=w, ckappa=0.5), 2 * 0.5 * u
    wl = w if per_point else w.view(1, N).expand(L, N)
    if ones:
        ref[1:] = 1.0 / (coef * dcu[1:] * wl[1:])
    cot = coef * dcu * ref * wl
    cot[L - 1] += base * ref[L - 1]
    return dict(res=dict(ref=ref, coef=coef, base=base, weak=weak)), cot.t().contiguous()


def _cot_job(arena, fields, u_dev, tag):
    """the job entries of _cot_host's fields, every tensor a guarded input; res.u: the forward's own output on the device"""
    if 'ubar' in fields:
        return dict(ubar=arena.inp(fields['ubar'], name='ubar' + tag))
    r = dict(fields['res'], u=u_dev)
    r['ref'] = arena.inp(r['ref'], name='res.ref' + tag)
    if 'weak' in r:
        r['weak'] = {k: (arena.inp(v, name='res.weak.%s%s' % (k, tag)) if torch.is_tensor(v) else v) for k, v in r['weak'].items()}
    return dict(res=r)


def _sweep_outputs(arena, d, N, P, slabs, mode, tag):
    """(gx, gs, gslab entries, the written ones, the untouched ones) of one sweep job in `mode`.  The slabs are followed, with no gap,
    by one slab more that holds -0.0: a 16-lane group entirely past N owns no slab, and lanes past N add zeros -- a read-modify-write
    of the slab behind the last one would leave a NaN guard as it is, but turns -0.0 into +0.0 (_check_beyond)"""
    big = arena.out(slabs + 1, P, name='gslab' + tag)
    big[slabs].fill_(-0.0)
    arena.__dict__.setdefault('beyond', []).append(big[slabs])
    o = dict(gx=arena.out(d, N, name='gx' + tag), gs=arena.out(N, name='gs' + tag), gslab=big[:slabs])
    want_x, want_params, _ = FLAGS[mode]
    xs, ps = [o['gx'], o['gs']], [o['gslab']]
    return o, (xs if want_x else []) + (ps if want_params else []), ([] if want_x else xs) + ([] if want_params else ps)


def _check_beyond(arena):
    """the slab behind every job's last one still holds -0.0 in every entry"""
    for i, v in enumerate(arena.beyond):
        bad = v.view(torch.int64) != -2 ** 63
        assert not bool(bad.any()), 'sweep job %d: %d entries of the slab behind its last one were touched (first: entry %d)' % (
            i, int(bad.sum()), int(torch.nonzero(bad)[0]))


def _same_bits(a, b, what):
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), '%s: not equal to the bit' % what


# ---- the generic stepper -----------------------------------------------------------------------------------------------------------
# The oracle's own rounding spread at the corners (oracle_spread below, float64, CPU): per case id (value spread: u, Y; gradient
# spread: gx, gs, every parameter's gradient and their sum).  A case is in the table when it is at the (64, 16) width or at
# u_layers = 32.
ORACLE_SPREAD = {
    'euler-params-res-N63+16-H64K16m11-d5-L3': (5.89e-16, 9.56e-16),
    'rk4-both-weak-N65-H20K10m32-d17-L1-noY': (4.33e-16, 6.25e-16),
    'midpoint-both_ones-res_first-N15+64-H20K10m32-d5-L1': (2.77e-16, 3.18e-16),
    'midpoint-x-res-N15-H5K3m32-d5-L1-noY': (2.57e-16, 2.22e-16),
    'euler-params-weak-N64+15-H20K10m32-d5-L1-noY': (5.12e-16, 1.13e-15),
    'rk4-both_ones-res-N64+15-H64K16m11-d5-L1-noY': (4.46e-16, 6.33e-16),
    'midpoint-params-res_first-N65+63-H33K9m32-d126-L3-noY': (3.17e-16, 5.81e-16),
    'euler-params-weak-N15+64-H5K3m32-d126-L3': (6.79e-16, 3.75e-16),
    'midpoint-x-res_first-N63-H64K16m32-d5-L2-noY': (7.04e-16, 9.35e-16),
    'euler-both-res_first-N1+17-H64K16m11-d126-L3-noY': (1.82e-16, 6.86e-16),
    'euler-x-weak-N63+16-H24K13m32-d1-L3': (2.74e-16, 1.31e-15),
    'rk4-params-ubar-N15-H64K16m11-d5-L2': (2.37e-15, 1.54e-15),
    'rk4-both_ones-ubar-N16-H64K16m32-d1-L3': (4.27e-16, 4.06e-15),
    'euler-both-weak-N17-H64K16m32-d1-L1-noY': (2.45e-16, 9.85e-16),
    'euler-params-res-N65-H64K16m32-d5-L1-noY': (4.26e-16, 5.39e-16),
    'euler-both-res-N64+15-H1K1m32-d17-L2': (0.00e+00, 7.27e-16),
}                                                   # (every spread is below an eighth of its tolerance: the project's stand)


def _corner(c):
    return (c['H'], c['K']) == (64, 16) or c['m'] == 32


def _tolerances(c):
    """(values, gradients): the project's, or 8 x the oracle's measured spread where that exceeds an eighth of them"""
    sv, sg = ORACLE_SPREAD[VI.gid(c)] if _corner(c) else (0.0, 0.0)
    return (8 * sv if sv > TOL_VALUE / 8 else TOL_VALUE), (8 * sg if sg > TOL_GRAD / 8 else TOL_GRAD)


def _generic_samples(c):
    """theta, its blob, t and per job (x, start)"""
    theta, blob = _theta(c['H'], c['K'], c['m'], c['d'], c['seed'])
    samples = [_sample(N, c['L'], c['d'], c['seed'] + 1000 + i) for i, N in enumerate(VI.generic_Ns(c))]
    return theta, blob, samples[0][1], [(x, s) for x, _, s, _ in samples]


def _compare_generic_sweep(KN, j, mode, theta, u_ref, leaves, cot, tol, what):
    want_x, want_params, ones = FLAGS[mode]
    want = E._grads(u_ref, leaves, cot)
    if want_x:
        wx = E._grads(u_ref, leaves, torch.ones_like(cot)) if ones else want
        _close(j['gx'].t(), wx[0], tol, what + ' gx')
        _close(j['gs'], wx[1], tol, what + ' gs')
    if want_params:
        E._check_params(KN.slab_sum(j['gslab']).cpu(), theta, want, tol, what)


@pytest.mark.parametrize('c', VI.GENERIC_CASES, ids=VI.gid)
def test_generic_stepper_paths(c):
    from xnode_wan_pde_solver_amd import kernels as KN
    method, mode, H, K, m, d, L = (c[k] for k in ('method', 'mode', 'H', 'K', 'm', 'd', 'L'))
    assert KN.ode_generic(H, K, m)                          # (a width / depth the C ABI hands to xw_generic.hip as it is)
    tol_v, tol_g = _tolerances(c)
    want_x, want_params, ones = FLAGS[mode]
    theta, blob, t, samples = _generic_samples(c)
    Ns = VI.generic_Ns(c)
    mid, P = KN.method_id(method), blob.numel()
    assert P == KN.theta_size(d, H, K)
    arena = G.Arena(torch.device(DEVICE))
    tc, bc = arena.inp(t, name='t'), arena.inp(blob, name='theta')
    ins = [dict(xT=arena.inp(x.t(), name='xT%d' % i), start=arena.inp(s, name='start%d' % i)) for i, (x, s) in enumerate(samples)]

    def fjob(i, tag, with_Y=True):
        j = dict(ins[i], u=arena.out(L, Ns[i], name='u%d%s' % (i, tag)))
        if with_Y:
            j['Y'] = arena.out(L, H, Ns[i], name='Y%d%s' % (i, tag))
        return j

    fjs = [fjob(i, '') for i in range(len(Ns))]
    KN.ode_fwd_multi(fjs, tc, bc, mid, H, K, m)
    written = [v for fj in fjs for v in (fj['u'], fj['Y'])]
    njs = []
    if not c['Y']:                                          # the same call without Y: the sweep below reads the first call's
        njs = [fjob(i, 'noY', with_Y=False) for i in range(len(Ns))]
        KN.ode_fwd_multi(njs, tc, bc, mid, H, K, m)
        written += [nj['u'] for nj in njs]
    cots = [_cot_host(c['cot'], ones, N, L, c['seed'] + 2000 + i, fjs[i]['u'].cpu()) for i, N in enumerate(Ns)]
    untouched = []

    def sjob(i, fj, tag):
        o, w_, u_ = _sweep_outputs(arena, d, Ns[i], P, KN.ode_bwd_slabs(Ns[i]), mode, '%d%s' % (i, tag))
        written.extend(w_)
        untouched.extend(u_)
        return dict(fj, **o, **_cot_job(arena, cots[i][0], fj['u'], '%d%s' % (i, tag))), w_

    sjs = [sjob(i, fj, '') for i, fj in enumerate(fjs)]
    KN.ode_bwd_multi([q for q, _ in sjs], tc, bc, mid, H, K, m, want_x=want_x, want_params=want_params, x_cot_ones=ones)
    alone = []
    if len(Ns) > 1:                                         # every job of the call once more, alone
        for i in range(len(Ns)):
            fa = fjob(i, 'alone')
            KN.ode_fwd_multi([fa], tc, bc, mid, H, K, m)
            written += [fa['u'], fa['Y']]
            sa = sjob(i, fa, 'alone')
            KN.ode_bwd_multi([sa[0]], tc, bc, mid, H, K, m, want_x=want_x, want_params=want_params, x_cot_ones=ones)
            alone.append((fa, sa))
    arena.check(written=written, untouched=untouched)
    _check_beyond(arena)
    for i, (fa, (_, wa)) in enumerate(alone):
        _same_bits(fa['u'], fjs[i]['u'], 'u of job %d alone' % i)
        _same_bits(fa['Y'], fjs[i]['Y'], 'Y of job %d alone' % i)
        for a_, b_ in zip(wa, sjs[i][1]):
            _same_bits(a_, b_, 'a sweep output of job %d alone' % i)
    for i, nj in enumerate(njs):
        _same_bits(nj['u'], fjs[i]['u'], 'u of job %d without Y' % i)
    for i, (x, s) in enumerate(samples):
        u_ref, Y_ref, leaves = E._oracle(theta, m, method, x, t, s)
        _close(fjs[i]['u'].t(), u_ref.detach(), tol_v, 'u job %d' % i)
        _close(fjs[i]['Y'], Y_ref, tol_v, 'Y job %d' % i)
        _compare_generic_sweep(KN, sjs[i][0], mode, theta, u_ref, leaves, cots[i][1], tol_g, '%s job %d' % (mode, i))


def oracle_spread(c):
    """(value spread, gradient spread) of a generic case's first job in _close's metric: the oracle as written against the oracle with
    the hidden units of both widths permuted and the paths in reverse order (test_gpu_edges.oracle_spread, for this file's cases)"""
    method, mode, H, K, m, d, L, N = (c[k] for k in ('method', 'mode', 'H', 'K', 'm', 'd', 'L', 'N'))
    theta, _, t, samples = _generic_samples(c)
    x, start = samples[0]
    u, Y, leaves = E._oracle(theta, m, method, x, t, start)
    _, cot = _cot_host(c['cot'], FLAGS[mode][2], N, L, c['seed'] + 2000, u.detach().t().contiguous())
    g = E._grads(u, leaves, cot)
    tp, ph, pk = E._permuted(theta, d, H, K, c['seed'] + 3000)
    rev = torch.arange(N - 1, -1, -1)
    u2, Y2, leaves2 = E._oracle(tp, m, method, x[rev].contiguous(), t, start[rev].contiguous())
    g2 = E._grads(u2, leaves2, cot[rev].contiguous())
    inv_h, inv_k = torch.argsort(ph), torch.argsort(pk)

    def rel(a, b):
        return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)

    sv = max(rel(u2.detach()[rev], u.detach()), rel(Y2[:, inv_h][:, :, rev], Y))
    un = [E._unpermuted(k, a, d, inv_h, inv_k) for k, a in zip(U_ORDER, g2[2:])]
    pairs = [(g2[0][rev], g[0]), (g2[1][rev], g[1])] + list(zip(un, g[2:]))
    pairs.append((torch.cat([a.reshape(-1) for a in un]), torch.cat([b.reshape(-1) for b in g[2:]])))
    return sv, max(rel(a, b) for a, b in pairs)


assert all(VI.gid(c) in ORACLE_SPREAD for c in VI.GENERIC_CASES if _corner(c)), 'ORACLE_SPREAD lacks a corner'
assert all(any(VI.gid(c) == k and _corner(c) for c in VI.GENERIC_CASES) for k in ORACLE_SPREAD)


# ---- the vector dopri5 -------------------------------------------------------------------------------------------------------------
def _dopri_samples(c):
    """cfg, theta, t [L] (float32 values as float64, t[1] = t[0] with dup) and per job (X [N, L, 1 + d], start)"""
    from test_gpu_dopri5 import _case
    d, H, K, m, L = (c[k] for k in ('d', 'H', 'K', 'm', 'L'))
    Ns = VI.dopri_Ns(c)
    cfg, theta, X0, s0 = _case(d, H, K, m, Ns[0], L, c['seed'])
    t = X0[0, :, 0].clone()
    if c['dup']:
        t[1] = t[0]
    samples = []
    for i, N in enumerate(Ns):
        X, s = (X0, s0) if i == 0 else _case(d, H, K, m, N, L, c['seed'] + 100 * i)[2:]
        X = X.clone()
        X[:, :, 0] = t.view(1, L)                           # (the jobs of a launch share t)
        samples.append((X, s * c['scale']))
    return cfg, theta, t.double(), samples


def _record_regions(rec):
    """(written, untouched) regions of a record after its forward"""
    n = rec.n_acc
    w = [rec.rec_y[:n + 1], rec.rec_t[:n + 1], rec.rec_h[:n], rec.work, rec.fbuf[0]]
    u = [rec.rec_y[n + 1:], rec.rec_t[n + 1:], rec.rec_h[n:]]
    (w if rec.n_att else u).append(rec.fbuf[1])
    return [v for v in w if v.numel()], [v for v in u if v.numel()]


def _own_widths(flat, d, H, K, Hc, Kc, m):
    """{key: the parameter's gradient at the network's own shape} from a summed slab laid out at (Hc, Kc); every entry of the blob
    that belongs to no parameter of the network -- padding units, the unused Wh slot of a tanh-only field -- must be exactly zero"""
    from xnode_wan_pde_solver_amd import nets
    slots, total = nets._u_slots(d, H, K, Hc, Kc, m > 1)
    assert total == flat.numel()
    keys = [k for k in U_ORDER if m > 1 or k not in ('Wh', 'Wh_b')]
    own = torch.zeros(total, dtype=torch.bool)
    out = {}
    for k, (off, r, c_, ld) in zip(keys, slots):
        out[k] = torch.stack([flat[off + i * ld:off + i * ld + c_] for i in range(r)])
        for i in range(r):
            own[off + i * ld:off + i * ld + c_] = True
    assert float(flat[~own].abs().sum()) == 0.0, 'a padding entry of the summed slab is not zero'
    return out


def _dopri_reference(theta, cfg, X, start, frozen):
    """u [N, L] (attached) on the frozen grid and the leaves (x, start, the parameters in U_ORDER)"""
    th = {k: v.clone().requires_grad_(True) for k, v in theta.items()}
    x64 = X[:, 0, 1:].double().clone().requires_grad_(True)
    s = start.clone().requires_grad_(True)
    N, L = X.shape[0], X.shape[1]
    Xd = torch.cat((X[:, :, :1].double(), x64.view(N, 1, -1).expand(N, L, -1)), 2)
    u, _ = D.u_net(th, cfg, Xd, s, frozen=frozen)
    return u, [x64, s] + [th[k] for k in U_ORDER]


def _compare_dopri_sweep(KN, j, mode, theta, dims, u_ref, leaves, cot, what):
    from test_gpu_dopri5 import _rel
    want_x, want_params, ones = FLAGS[mode]
    want = E._grads(u_ref, leaves, cot)
    if want_x:
        wx = E._grads(u_ref, leaves, torch.ones_like(cot)) if ones else want
        for name, got, ref in (('gx', j['gx'].t(), wx[0]), ('gs', j['gs'], wx[1])):
            print(what, name, _rel(got, ref))
            assert _rel(got, ref) < DOPRI_TOL, (what, name, _rel(got, ref))
    if want_params:
        got = _own_widths(KN.slab_sum(j['gslab']).cpu(), *dims)
        ref = dict(zip(U_ORDER, want[2:]))
        for k, v in got.items():
            r = _rel(v.reshape(ref[k].shape), ref[k])
            assert r < DOPRI_TOL, (what, k, r)
        r = _rel(torch.cat([v.reshape(-1) for v in got.values()]), torch.cat([ref[k].reshape(-1) for k in got]))
        print(what, 'parameter gradient', r)
        assert r < DOPRI_TOL, (what, 'summed parameter gradient', r)


def _run_dopri(c):
    from test_gpu_dopri5 import GRID_TOL, _blob, _grid_of, _ref_Y, _rel
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m, L, mode = (c[k] for k in ('d', 'H', 'K', 'm', 'L', 'mode'))
    want_x, want_params, ones = FLAGS[mode]
    cfg, theta, t, samples = _dopri_samples(c)
    Ns = VI.dopri_Ns(c)
    blob, Hc, Kc = _blob(theta, d, H, K, m)
    assert (Hc, Kc) == KN.ode_container(H, K, m) and c['inst'] in (None, VI.instantiation(Hc))
    P = blob.numel()
    assert P == KN.theta_size(d, Hc, Kc)
    kw = dict(cap=2, chunk=3) if c['grow'] else {}
    arena = G.Arena(torch.device(DEVICE))
    tc, bc = arena.inp(t, name='t'), arena.inp(blob, name='theta')
    ins = [dict(xT=arena.inp(X[:, 0, 1:].double().t(), name='xT%d' % i), start=arena.inp(s, name='start%d' % i))
           for i, (X, s) in enumerate(samples)]
    written, untouched = [], []

    def forward(idx, tag):
        fjs = [dict(ins[i], u=arena.out(L, Ns[i], name='u%d%s' % (i, tag)), Y=arena.out(L, Hc, Ns[i], name='Y%d%s' % (i, tag))) for i in idx]
        recs = KN.dopri5_fwd(fjs, tc, bc, Hc, Kc, m, H, stepper='vector', **kw)
        for fj, rec in zip(fjs, recs):
            w_, u_ = _record_regions(rec)
            written.extend([fj['u'], fj['Y']] + w_)
            untouched.extend(u_)
        return fjs, recs

    def sweep(idx, fjs, recs, tag):
        sjs = []
        for i, fj, rec in zip(idx, fjs, recs):
            o, w_, u_ = _sweep_outputs(arena, d, Ns[i], P, KN.ode_bwd_slabs(Ns[i]), mode, '%d%s' % (i, tag))
            written.extend(w_)
            untouched.extend(u_)
            sjs.append((dict(ins[i], rec=rec, **o, **_cot_job(arena, cots[i][0], fj['u'], '%d%s' % (i, tag))), w_))
        KN.dopri5_sweep([q for q, _ in sjs], tc, bc, Hc, Kc, m, want_x=want_x, want_params=want_params, x_cot_ones=ones, stepper='vector')
        return sjs

    every = list(range(len(Ns)))
    with arena.dopri5_records(KN):
        fjs, recs = forward(every, '')
        fjs2, recs2 = forward(every, 'again')
        cots = [_cot_host(c['cot'], ones, N, L, c['seed'] + 2000 + i, fjs[i]['u'].cpu()) for i, N in enumerate(Ns)]
        sjs = sweep(every, fjs, recs, '')
        alone = []
        if len(Ns) > 1:
            for i in every:
                fa, ra = forward([i], 'alone')
                alone.append((fa[0], ra[0], sweep([i], fa, ra, 'alone')[0]))
    arena.check(written=written, untouched=untouched)
    _check_beyond(arena)
    for i in every:
        a, b = recs[i], recs2[i]
        assert (a.n_att, a.n_acc) == (b.n_att, b.n_acc) and torch.equal(a.grid, b.grid), 'job %d: the second run took other steps' % i
        _same_bits(fjs[i]['u'], fjs2[i]['u'], 'u of job %d, second run' % i)
        _same_bits(fjs[i]['Y'], fjs2[i]['Y'], 'Y of job %d, second run' % i)
        _same_bits(a.rec_y[:a.n_acc + 1], b.rec_y[:a.n_acc + 1], 'the recorded states of job %d, second run' % i)
        assert a.cap >= a.n_acc and (not c['grow'] or a.cap > 2)
    for i, (fa, ra, (_, wa)) in enumerate(alone):
        assert (ra.n_att, ra.n_acc) == (recs[i].n_att, recs[i].n_acc) and torch.equal(ra.grid, recs[i].grid), 'job %d alone' % i
        _same_bits(fa['u'], fjs[i]['u'], 'u of job %d alone' % i)
        _same_bits(fa['Y'], fjs[i]['Y'], 'Y of job %d alone' % i)
        for a_, b_ in zip(wa, sjs[i][1]):
            _same_bits(a_, b_, 'a sweep output of job %d alone' % i)
    for i, (X, s) in enumerate(samples):
        rec, fj = recs[i], fjs[i]
        if c['exact']:
            ys, info = _ref_Y(theta, cfg, X, s)
            assert info['gap'] > 1e-9, 'bad fixture: a step decision within %.1e of the threshold' % info['gap']
            print('device', (rec.n_att, rec.n_acc), 'restatement', (info['n_att'], info['n_acc']), 'gap', info['gap'])
            assert (rec.n_att, rec.n_acc) == (info['n_att'], info['n_acc'])
            grid_tol = E._grid_tolerance(info, GRID_TOL) if Ns[i] == 1 else GRID_TOL
            print('grid', _rel(rec.grid, _grid_of(info)), 'bound', grid_tol)
            assert _rel(rec.grid, _grid_of(info)) < grid_tol
        else:
            ys, _ = _ref_Y(theta, cfg, X, s, frozen=rec.steps)
            assert rec.n_att >= rec.n_acc and (rec.n_acc > 0) == bool(t[-1] > t[0])
        if c['dup']:
            _same_bits(fj['u'][1], fj['u'][0], 'u at t[1] == t[0]')
        u_ref = (ys @ theta['FL_w'].T + theta['FL_b']).squeeze(2)
        print('job', i, 'u', _rel(fj['u'].t(), u_ref), 'Y', _rel(fj['Y'][:, :H, :].permute(2, 0, 1), ys))
        assert _rel(fj['u'].t(), u_ref) < DOPRI_TOL
        assert _rel(fj['Y'][:, :H, :].permute(2, 0, 1), ys) < DOPRI_TOL
        if Hc > H:
            assert float(fj['Y'][:, H:, :].abs().max()) == 0.0, 'the padding units do not stay exactly zero'
        u_r, leaves = _dopri_reference(theta, cfg, X, s, rec.steps)
        _compare_dopri_sweep(KN, sjs[i][0], mode, theta, (d, H, K, Hc, Kc, m), u_r, leaves, cots[i][1], '%s job %d' % (mode, i))
    return recs


@pytest.mark.parametrize('c', VI.DOPRI_COVER, ids=VI.did)
def test_vector_dopri5_paths(c):
    _run_dopri(c)


@pytest.mark.parametrize('c', VI.DOPRI_EXACT, ids=VI.did)
def test_vector_dopri5_exact_step_decisions(c):
    rec, = _run_dopri(c)
    if c['counts'] is not None:
        assert (rec.n_att, rec.n_acc) == c['counts']
    if (c['seed'], c['scale']) in VI.REJECTING:
        assert rec.n_att > rec.n_acc


def test_nine_jobs_raise():
    """the limit of eight jobs per call, on the vector stepper's wrappers (the eight-job calls themselves: the covering cases)"""
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    dev = torch.device(DEVICE)
    d, H, K, m, L, N = 2, 33, 9, 11, 2, 3
    _, blob = _theta(H, K, m, d, 5)
    x, t, start, _ = _sample(N, L, d, 6)
    jobs = [dict(xT=x.t().contiguous().to(dev), start=start.to(dev), u=torch.empty(L, N, dtype=F64, device=dev)) for _ in range(9)]
    with pytest.raises(XnwanError, match='1 .. 8 jobs'):
        KN.dopri5_fwd(jobs, t.to(dev), blob.to(dev), H, K, m, H, stepper='vector')
    rec, = KN.dopri5_fwd(jobs[:1], t.to(dev), blob.to(dev), H, K, m, H, stepper='vector')
    with pytest.raises(XnwanError, match='1 .. 8 jobs'):
        KN.dopri5_sweep([dict(j, rec=rec) for j in jobs], t.to(dev), blob.to(dev), H, K, m, True, False, stepper='vector')


# ---- the tail that exists twice ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,K,m,N,d', VI.TAIL_CASES)
def test_both_copies_of_the_sweep_tail(H, K, m, N, d):
    """L = 1: kg_ode_bwd and kd_sweep run nothing but the l = 0 read-out and lift tail, which each holds a copy of.  The same inputs
    through both, every sweep mode and cotangent form: every output against the oracle, and the two results against each other"""
    from test_gpu_dopri5 import _rel
    from xnode_wan_pde_solver_amd import kernels as KN
    L, seed = 1, 1700 + H
    assert KN.ode_container(H, K, m) == (H, K) and KN.ode_generic(H, K, m)      # (both families at the network's own widths)
    theta, blob = _theta(H, K, m, d, seed)
    x, t, start, _ = _sample(N, L, d, seed + 1)
    P = blob.numel()
    arena = G.Arena(torch.device(DEVICE))
    tc, bc = arena.inp(t, name='t'), arena.inp(blob, name='theta')
    ins = dict(xT=arena.inp(x.t(), name='xT'), start=arena.inp(start, name='start'))
    written, untouched = [], []
    gj = dict(ins, u=arena.out(L, N, name='u.generic'), Y=arena.out(L, H, N, name='Y.generic'))
    dj = dict(ins, u=arena.out(L, N, name='u.dopri5'), Y=arena.out(L, H, N, name='Y.dopri5'))
    KN.ode_fwd_multi([gj], tc, bc, KN.method_id('euler'), H, K, m)
    with arena.dopri5_records(KN):
        rec, = KN.dopri5_fwd([dj], tc, bc, H, K, m, H, stepper='vector')
    assert (rec.n_att, rec.n_acc) == (0, 0) and rec.steps == []              # (nothing to integrate: the controller starts done)
    w_, u_ = _record_regions(rec)
    written += [gj['u'], gj['Y'], dj['u'], dj['Y']] + w_
    untouched += u_
    u_host = gj['u'].cpu()
    runs = []
    for mode in VI.MODES:
        for k, form in enumerate(VI.COTS):
            want_x, want_params, ones = FLAGS[mode]
            fields, cot = _cot_host(form, ones, N, L, seed + 10 + k, u_host)
            pair = []
            for fam, fj in (('generic', gj), ('dopri5', dj)):
                tag = '.%s.%s.%s' % (fam, mode, form)
                o, wr, un = _sweep_outputs(arena, d, N, P, KN.ode_bwd_slabs(N), mode, tag)
                written += wr
                untouched += un
                j = dict(fj, **o, **_cot_job(arena, fields, fj['u'], tag))
                if fam == 'generic':
                    KN.ode_bwd_multi([j], tc, bc, KN.method_id('euler'), H, K, m, want_x=want_x, want_params=want_params, x_cot_ones=ones)
                else:
                    KN.dopri5_sweep([dict(j, rec=rec)], tc, bc, H, K, m, want_x=want_x, want_params=want_params, x_cot_ones=ones,
                                    stepper='vector')
                pair.append((j, wr))
            runs.append((mode, form, cot, pair))
    arena.check(written=written, untouched=untouched)
    _check_beyond(arena)
    u_ref, Y_ref, leaves = E._oracle(theta, m, 'euler', x, t, start)
    _same_bits(gj['u'], dj['u'], 'u of the two families')
    _same_bits(gj['Y'], dj['Y'], 'Y of the two families')
    _close(gj['u'].t(), u_ref.detach(), TOL_VALUE, 'u')
    _close(gj['Y'], Y_ref, TOL_VALUE, 'Y')
    worst = 0.0
    for mode, form, cot, ((g_, gw), (d_, dw)) in runs:
        what = '%s %s' % (mode, form)
        _compare_generic_sweep(KN, g_, mode, theta, u_ref, leaves, cot, TOL_GRAD, 'kg_ode_bwd ' + what)
        _compare_dopri_sweep(KN, d_, mode, theta, (d, H, K, H, K, m), u_ref, leaves, cot, 'kd_sweep ' + what)
        for a_, b_ in zip(gw, dw):                          # (gx, gs, the slabs as stored: both give a 16-path group the same slab)
            worst = max(worst, _rel(a_, b_))
            _close(a_, b_, TAIL_TOL, 'the two copies of the tail, ' + what)
    print('the two copies differ by at most %.2e (bound %.2e)' % (worst, TAIL_TOL))


if __name__ == '__main__':
    print('cases: generic stepper %d, vector dopri5 %d covering + %d exact, tail %d' % (
        len(VI.GENERIC_CASES), len(VI.DOPRI_COVER), len(VI.DOPRI_EXACT), len(VI.TAIL_CASES)))
    print('| case | value spread | gradient spread | tolerance (values, gradients) |')
    for c_ in VI.GENERIC_CASES:
        if _corner(c_):
            sv_, sg_ = oracle_spread(c_)
            print('| %s | %.2e | %.2e | %s |' % (VI.gid(c_), sv_, sg_, (8 * sv_ if sv_ > TOL_VALUE / 8 else TOL_VALUE,
                                                                       8 * sg_ if sg_ > TOL_GRAD / 8 else TOL_GRAD)))
