"""The weak-form, cotangent, loss and Adam kernels (csrc/xw_weak.hip: k_weak_partials with the deterministic grid_sum, k_bdry,
k_gen_cots, k_disc_cot, k_losses, k_pair_fold, k_adam) against the oracle at edge shapes, inside a guard-banded, poisoned arena.

The reference side is tests/weak_ref.py: the kernels' operands mapped onto oracle/refspec.py's own functions (float64, CPU, every
cotangent by autograd), every reduced scalar with the exact sum (math.fsum) of the terms that were added and their sum_abs.  The
case tables live there too, with the coverage they assert: every listed value of every mode axis occurs with every shape regime
(L > d, L = d, L < d with a ragged stride, pairwise), every listed shape occurs; Adam: every listed value of every axis.  (href and
an s3_scale other than 1 are arguments of the pairwise form only -- kernels.weak_partials(pair=dict(href, s3_scale)) -- and are
covered there; the two large shapes are single launches, the two-launch accumulation runs at the smaller ones.)

Every case
  * takes every operand from one guarded.Arena: scal, work, the step / lag counters (one double each, viewed as int64, between guard
    bands), outputs pre-filled with the NaN pattern.  `work` cannot hold the pattern (its ticket word must be zero): it is zeroed, and
    the doubles behind xw_reduce_work_size() are the arena's guard band;
  * after the launches calls Arena.check once: no guard changed, every output element written, and what the kernels leave alone by
    design still the pattern -- scal[9:], scal[4:7] without a finalisation, scal[7:9] outside pairwise groups (the launch adds its zero
    partial sums to them: a NaN keeps its bits); under `skip` the lagged range of param / m / v holds the bits it held;
  * launches every xw_weak_partials sequence twice into two scal buffers: the results must be bitwise equal.

Tolerances (tests/weak_ref.py): reduced scalars scal[0..3, 7, 8]: |got - exact| <= 1e-13 x sum_abs -- each term takes about a dozen
roundings and the fixed tree adds about 30 (three serial trips, six wave levels, 16 waves, the block-order pass): 1e-14 x sum_abs, a
factor of 10 left; one dropped term of 270,435 is 4e-6 x sum_abs.  Loss values scal[4..6]: rtol 1e-11, on inputs with
|I| >= 1e-2 x sum_abs (asserted on the reference side).  Elementwise outputs and Adam: 1e-13 in _close's metric; the cotangents are
compared per time row group (l = 0, where the alpha-weighted initial penalty sets the scale, apart from l > 0).

Launch shapes (csrc/xw_weak.hip reduce_cap / reduce_threads): 1024 threads; 128 blocks up to 2^18 points, 256 above.  (4099, 33, 4)
is 135,267 points: a second grid-stride trip; (8195, 33, 4) is 270,435: the 256-block cap.  The library switches reduce_threads=256
with reduce_blocks=3 (four waves per block, three blocks, many trips): the small shapes' cases once more, through the same case
function, inside kernels.switched(...).

`python tests/test_gpu_weak.py` (CPU only) prints the case tables and the reference-vs-exact gaps.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import guarded as G  # noqa: E402
import weak_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
DEVICE = 'cuda'
ORACLE_SPREAD = W.ORACLE_SPREAD


def _counter(arena, value, name):
    """an int64 counter in one double of the arena (its neighbours are guard bands)"""
    t = arena.out(1, name=name).view(torch.int64)
    t.fill_(value)
    return t


def _work(arena, KN, name='work'):
    w = arena.out(KN.reduce_work_size(), name=name)
    w.zero_()
    return w


def _scal(arena, pair, name='scal'):
    """scal[16]: the sums' slots zeroed (the launches ADD), everything else the pattern"""
    s = arena.out(16, name=name)
    s[0:4] = 0.0
    if pair:
        s[7:9] = 0.0
    return s


def _scal_masks(c, final):
    idx = torch.arange(16)
    written = (idx < 4) | (((idx >= 4) & (idx < 7)) if final else torch.zeros(16, dtype=torch.bool))
    if c['pair']:
        written |= (idx == 7) | (idx == 8)
    return written, ~written


def _const_scal(arena, values, name):
    t = torch.full((16,), float('nan'), dtype=F64)
    t[:len(values)] = torch.tensor(values, dtype=F64)
    return arena.inp(t, name=name)


class _Shard:
    """the device operands of one launch of a case: paths [lo, hi) of the batch"""

    def __init__(self, arena, KN, c, o, lo, hi):
        cut = lambda x: None if x is None else arena.inp(x[..., lo:hi].contiguous())      # noqa: E731
        self.n = hi - lo
        for k in ('u', 'v', 'vt', 'wt', 'f', 'h', 'href', 'w', 'w0', 'gx', 'gs', 'ghT', 'gxv', 'gwx0T', 'c', 'cp'):
            setattr(self, k, cut(o[k]))
        self.contract, self.s3x = None, None
        if c['grad'] == 's3x':
            self.s3x = arena.out(self.n, name='s3x')
            KN.weak_contract_general(cut(o['a0']), 3, cut(o['b0']), self.gx, self.gs, self.ghT, self.gxv, self.w0, self.gwx0T,
                                     self.v[0], self.s3x)
        else:
            self.contract = dict(gx=self.gx, gs=self.gs, ghT=self.ghT, gxv=self.gxv, w0=self.w0, gwx0T=self.gwx0T)


def _launch_weak(KN, c, o, sh, N, scal, work, finalize=None, bdry=None):
    pair = dict(href=sh.href, s3_scale=o['s3_scale']) if c['pair'] else None
    KN.weak_partials(sh.u, sh.v, sh.vt, sh.w, sh.f, sh.h, W.VOL, float(N), scal, work, s3x=sh.s3x, contract=sh.contract, c=sh.c,
                     ckappa=W.KAPPA, wt=sh.wt, finalize=finalize, pair=pair, bdry=bdry)


def run_case(c):
    from xnode_wan_pde_solver_amd import kernels as KN
    o, r = W.inputs(c), W.reference(c)
    N, L, d = c['shape']
    dev = torch.device(DEVICE)
    arena = G.Arena(dev)
    parts = [_Shard(arena, KN, c, o, lo, hi) for lo, hi in W.shards(c)]
    works = [_work(arena, KN, 'work%d' % i) for i in range(len(parts))]
    final = c['final'] != 'none'
    ub = arena.inp(o['ub'], name='ub') if o['ub'] is not None else None
    gb = arena.inp(o['gb'], name='gb') if o['ub'] is not None else None
    Lb, Nb = o['ub'].shape if o['ub'] is not None else (1, 1)
    work_b = _work(arena, KN, 'work_b') if c['bdry'] == 'launch' else None
    ubar_b = arena.out(Lb, Nb, name='ubar_b') if c['bdry'] == 'launch' else None
    step = _counter(arena, 5, 'step')
    fz = dict(Lb=Lb, Nbglob=float(Nb), alpha=W.ALPHA, step=step, init_off=o['init_off'], bdry_off=o['bdry_off'])

    def sequence(scal):
        if c['bdry'] == 'launch':
            KN.bdry_partials(ub, gb, W.ALPHA, float(Nb), scal, work_b, ubar_b=ubar_b)
        for i, (sh, wk) in enumerate(zip(parts, works)):
            _launch_weak(KN, c, o, sh, N, scal, wk, finalize=fz if c['final'] == 'kernel' else None,
                         bdry=dict(ub=ub, g=gb) if (i == 0 and c['bdry'] in ('pb1', 'pbNL', 'pbGT')) else None)

    scal, scal2 = _scal(arena, c['pair'], 'scal'), _scal(arena, c['pair'], 'scal2')
    sequence(scal)
    sequence(scal2)
    sums = scal.cpu().clone()                                                    # (the sums as the launches left them)
    assert torch.equal(sums.view(torch.int64), scal2.cpu().view(torch.int64)), 'two runs of the same launches differ: %s | %s' % (
        sums[:9].tolist(), scal2.cpu()[:9].tolist())
    if c['final'] == 'split':
        if c['pair']:
            KN.pair_fold(scal, W.VOL, float(N))
        KN.losses(scal, L, Lb, W.VOL, float(N), float(Nb), W.ALPHA, step=step, init_off=o['init_off'], bdry_off=o['bdry_off'])
    # ---- the cotangents: per launch, with Nglob the whole batch; the global I and S come from the reference ----
    scal_d = _const_scal(arena, [r['I'].value, r['S'].value], 'scal_d')
    outs = []
    for sh in parts:
        sh.vbar = arena.out(L, sh.n, name='vbar')
        KN.disc_cotangent(sh.u, sh.v, sh.w, sh.f, sh.h, W.VOL, float(N), scal_d, sh.vbar, c=sh.c, ckappa=W.KAPPA,
                          pollution=c['pollution'], s3_scale=o['s3_scale'])
        outs.append(sh.vbar)
        if not c['pair']:
            scal_g = _const_scal(arena, [r['I_gen']], 'scal_g')
            sh.A, sh.B, sh.M = (arena.out(L, sh.n, name=k) for k in ('ubarA', 'ubarB', 'merged'))
            KN.gen_cotangents(sh.u, sh.v, sh.w, sh.h, W.VOL, float(N), W.ALPHA, sh.A, sh.B, c=sh.c, cp=sh.cp, ckappa=W.KAPPA,
                              pollution=c['pollution'])
            KN.gen_cotangents(sh.u, sh.v, sh.w, sh.h, W.VOL, float(N), W.ALPHA, sh.M, None, c=sh.c, cp=sh.cp, ckappa=W.KAPPA,
                              pollution=c['pollution'], scal=scal_g)
            # (one basis at a time: A alone does not read the test network at all)
            sh.A1, sh.B1 = arena.out(L, sh.n, name='ubarA alone'), arena.out(L, sh.n, name='ubarB alone')
            KN.gen_cotangents(sh.u, None, sh.w, sh.h, W.VOL, float(N), W.ALPHA, sh.A1, None, c=sh.c, cp=sh.cp,
                              ckappa=W.KAPPA, pollution=c['pollution'])
            KN.gen_cotangents(sh.u, sh.v, sh.w, sh.h, W.VOL, float(N), W.ALPHA, None, sh.B1, c=sh.c, cp=sh.cp, ckappa=W.KAPPA,
                              pollution=c['pollution'])
            outs += [sh.A, sh.B, sh.M, sh.A1, sh.B1]
    wr, un = _scal_masks(c, final)
    wr2, un2 = _scal_masks(c, c['final'] == 'kernel')
    arena.check(written=outs + [(scal, wr), (scal2, wr2)] + ([ubar_b] if ubar_b is not None else []) + [p.s3x for p in parts if p.s3x is not None],
                untouched=[(scal, un), (scal2, un2)])
    for wk in works + ([work_b] if work_b is not None else []):
        tail = wk[6 * 1024:].cpu()
        assert float(tail.abs().max()) == 0.0, 'the ticket word and the spare doubles of work are zero after the launches'
    # the step counter: once per finalising launch (twice: the sequence ran twice), once by losses
    assert int(step.item()) == 5 + {'none': 0, 'kernel': 2, 'split': 1}[c['final']], int(step.item())
    W.check_weak_scal(c, sums, 'final' if c['final'] == 'kernel' else 'sums')
    if c['final'] == 'split':
        W.check_weak_scal(c, scal.cpu(), 'final')
    lo = 0
    for sh in parts:
        s = slice(lo, lo + sh.n)
        lo += sh.n
        rows = [slice(0, 1)] + ([slice(1, L)] if L > 1 else [])
        for rw in rows:
            what = '%s paths %d.. rows %s ' % (W.wid(c), s.start, rw)
            W.close(sh.vbar[rw], r['vbar'][rw, s], W.TOL_ELEM, what + 'vbar')
            if not c['pair']:
                W.close(sh.A[rw], r['ubarA'][rw, s], W.TOL_ELEM, what + 'ubarA')
                W.close(sh.B[rw], r['ubarB'][rw, s], W.TOL_ELEM, what + 'ubarB')
                W.close(sh.M[rw], r['merged'][rw, s], W.TOL_ELEM, what + 'merged cotangent')
                assert torch.equal(sh.A1[rw], sh.A[rw]) and torch.equal(sh.B1[rw], sh.B[rw]), what + 'one basis alone'
    if ubar_b is not None:
        W.close(ubar_b, r['ubar_b'], W.TOL_ELEM, W.wid(c) + ' ubar_b')


@pytest.mark.parametrize('c', W.WEAK_CASES, ids=W.wid)
def test_weak_form_against_the_oracle(c):
    run_case(c)


# ---- the workspace contract --------------------------------------------------------------------------------------------------------------
def _plain_case(shape):
    return next(c for c in W.WEAK_CASES if c['shape'] == shape and not c['pair'])


def test_workspace_contract():
    """ONE zero-initialised `work` for launches of different grid sizes and NV, in order: weak_partials at (4099, 33, 4) [128 blocks x 6
    values], bdry_partials at (Nb, Lb) = (300, 3) [1 block x 1 value], weak_partials at (37, 7, 5) [1 block x 6], weak_partials at
    (4099, 33, 4) again.  Each result equals, bit for bit, the same launch on a fresh zeroed buffer, and matches the oracle.  (With the
    ticket at work[gridDim.x * NV] the second launch found its ticket word on a stale partial sum and left scal as it was.)"""
    from oracle import refspec as R
    from xnode_wan_pde_solver_amd import kernels as KN
    dev = torch.device(DEVICE)
    arena = G.Arena(dev)
    big, small = _plain_case((4099, 33, 4)), _plain_case((37, 7, 5))
    g = torch.Generator().manual_seed(77)
    ubh, gbh = torch.randn(3, 300, generator=g, dtype=F64), torch.randn(3, 300, generator=g, dtype=F64)
    bref = W.Sum(R.bdry_loss(ubh, gbh) * ubh.numel(), [(ubh - gbh) ** 2])
    ub, gb = arena.inp(ubh, name='ub'), arena.inp(gbh, name='gb')
    ops = {id(c): (_Shard(arena, KN, c, W.inputs(c), 0, c['shape'][0]), W.inputs(c)) for c in (big, small)}
    shared = _work(arena, KN, 'shared work')

    def launch(step, work, name):
        scal = _scal(arena, False, name)
        if step == 'bdry':
            KN.bdry_partials(ub, gb, W.ALPHA, 300.0, scal, work)
        else:
            sh, o = ops[id(step)]
            _launch_weak(KN, step, o, sh, step['shape'][0], scal, work)
        return scal

    results = []
    for i, step in enumerate((big, 'bdry', small, big)):
        got = launch(step, shared, 'scal shared %d' % i).cpu()
        fresh = launch(step, _work(arena, KN, 'fresh work %d' % i), 'scal fresh %d' % i).cpu()
        print('launch %d: shared %s fresh %s' % (i + 1, got[:4].tolist(), fresh[:4].tolist()))
        assert torch.equal(got.view(torch.int64), fresh.view(torch.int64)), 'launch %d on the shared workspace: %s, on a fresh one: %s' % (
            i + 1, got[:4].tolist(), fresh[:4].tolist())
        if step == 'bdry':
            W.check_sum('launch %d SSE bdry' % (i + 1), got[3], bref)
        else:
            r = W.reference(step)
            W.check_sum('launch %d I' % (i + 1), got[0], r['I'])
            W.check_sum('launch %d sum v^2' % (i + 1), got[1], r['S'])
            W.check_sum('launch %d SSE init' % (i + 1), got[2], r['sse_init'])
        results.append(got)
    assert torch.equal(results[0].view(torch.int64), results[3].view(torch.int64))
    arena.check()
    assert float(shared[6 * 1024:].abs().max()) == 0.0


# ---- the process-wide launch-shape switches --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', W.SMALL_CASES, ids=W.wid)
def test_small_shapes_with_three_blocks_of_four_waves(c):
    """the small shapes' cases under the library switches reduce_threads=256, reduce_blocks=3"""
    from xnode_wan_pde_solver_amd import kernels as KN
    with KN.switched(reduce_threads=256, reduce_blocks=3):
        assert (KN.switches()['reduce_threads'], KN.switches()['reduce_blocks']) == (256, 3)
        run_case(c)


# ---- Adam --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', W.ADAM_CASES, ids=W.aid)
def test_adam_against_the_oracle(c):
    """four updates (skip, skip, update, update where there is a lagged range): param, m, v per segment after every update, the summed
    gradient, exact step / lag counters, the lagged range bit for bit under skip"""
    from xnode_wan_pde_solver_amd import kernels as KN
    r = W.adam_reference(c)
    P = c['P']
    lo, hi = W.lag_range(c)
    arena = G.Arena(torch.device(DEVICE))
    param, m, v = arena.inp(r['p0'], name='param'), arena.inp(torch.zeros(P, dtype=F64), name='m'), arena.inp(torch.zeros(P, dtype=F64), name='v')
    step, lag = _counter(arena, 0, 'step'), (_counter(arena, 0, 'lag') if hi > lo else None)
    scal_l = _scal(arena, False, 'scal of losses')                               # (bump_step False / -1: xw_losses advances the counter)
    scal_l[0:4] = torch.tensor([2.0, 3.0, 1.0, 1.0], dtype=F64)
    written = []
    for it, up in enumerate(r['updates']):
        dv = lambda x, n: None if x is None else arena.inp(x, name='%s%d' % (n, it))      # noqa: E731
        A, B, eA, eB = dv(up['A'], 'slabA'), dv(up['B'], 'slabB'), dv(up['eA'], 'extraA'), dv(up['eB'], 'extraB')
        scal = _const_scal(arena, [up['I']], 'scal%d' % it) if c['scal'] else None
        gsum = {'none': None, 'own': arena.out(P, name='gsum%d' % it), 'alias': eA}[c['gsum']]
        before = (param.cpu().clone(), m.cpu().clone(), v.cpu().clone())
        advance = lambda: KN.losses(scal_l, 1, 1, W.VOL, 1.0, 1.0, W.ALPHA, step=step)   # noqa: E731
        if c['bump'] == -1:
            advance()
        KN.adam(param, A, m, v, step, W.LR, gextraA=eA, gslabB=B, gextraB=eB, scal=scal, gsum_out=gsum, bump_step=c['bump'],
                lag=lag, lag_range=(lo, hi), skip=up['skip'])
        if c['bump'] is False:
            advance()
        assert int(step.item()) == it + 1
        W.check_adam(c, it, param, m, v, gsum=gsum, before=before)
        if c['gsum'] == 'own':
            written.append(gsum)
    assert int(step.item()) == r['step'] and (lag is None or int(lag.item()) == r['lag'])
    arena.check(written=written, untouched=[(scal_l, torch.arange(16) >= 7)])


if __name__ == '__main__':
    print('| weak-form case | points | launches | I: abs(oracle - exact) / sum_abs | abs(I) / sum_abs | worst gap of the other sums |')
    for c_ in W.WEAK_CASES:
        r_ = W.reference(c_)
        sums_ = [v_ for v_ in r_.values() if isinstance(v_, W.Sum)]
        print('| %s | %d | %d | %.1e | %.2e | %.1e |' % (W.wid(c_), c_['shape'][0] * c_['shape'][1], len(W.shards(c_)), r_['I'].gap(),
                                                         abs(r_['I'].exact) / r_['I'].sum_abs, max(s_.gap() for s_ in sums_ if s_ is not r_['I'])))
    print('ORACLE_SPREAD entries: %d' % len(ORACLE_SPREAD))
    print('| Adam case |')
    for c_ in W.ADAM_CASES:
        print('| %s |' % W.aid(c_))
