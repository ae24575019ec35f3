"""CPU tests of the reference side of tests/test_gpu_weak.py (tests/weak_ref.py): no GPU.

  * The reference alone: for every case of the GPU module, the float64 oracle and the exact sum (math.fsum) of the same terms differ
    by at most 1e-14 x sum_abs -- a tenth of the GPU tolerance -- for every reduced scalar; finalised cases have |I| >= 1e-2 x sum_abs.
  * The pairwise factorisation the caller is asked to perform (s3_scale = Nglob, f := mean f, href := mean h, init_off = var h; the
    boundary mean likewise) against R.weak_I_shaped / the pairwise means as R.group_forward writes them.
  * The comparison bites: plain-torch stand-ins of the kernels' outputs (below; the ONLY place where the kernels' formulas are typed
    again, and only to be broken) pass the module's comparison helpers as they are and fail them under each mutation.
  * The case tables cover what they claim (asserted on import of tests/weak_ref.py; restated here), ORACLE_SPREAD is consistent.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402
import weak_ref as W  # noqa: E402

F64 = torch.float64


# ---- the reference alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', W.WEAK_CASES, ids=W.wid)
def test_oracle_agrees_with_the_exact_sum_of_its_terms(c):
    r = W.reference(c)
    sums = {k: v for k, v in r.items() if isinstance(v, W.Sum)}
    assert {'I', 'S', 'sse_init'} <= set(sums) and ('sse_bdry' in sums) == (c['bdry'] != 'none')
    for k, s in sums.items():
        print('%s %s: oracle %.17g exact %.17g gap %.2e x sum_abs' % (W.wid(c), k, s.value, s.exact, s.gap()))
        assert s.sum_abs > 0 and s.gap() <= W.TOL_REF, (k, s.gap())
    if c['final'] != 'none':
        assert W.well_conditioned(c), abs(r['I'].exact) / r['I'].sum_abs
    assert all(math.isfinite(r[k]) for k in ('loss_u', 'loss_v', 'int'))


def test_case_tables_cover_what_they_claim():
    assert not W.missing(W.WEAK_CASES)
    for ax, vals in W.AXES.items():
        for v in vals:
            for reg in W.REGIMES:
                if reg != 'pair' and ((ax == 'href' and v) or (ax == 's3' and v == 'N')):
                    continue                                                     # (both only exist in the pairwise form)
                assert any(c[ax] == v and c['regime'] == reg for c in W.WEAK_CASES), (ax, v, reg)
    assert {c['shape'] for c in W.WEAK_CASES if not c['pair']} == set(W.NONPAIR)
    assert {c['shape'] for c in W.WEAK_CASES if c['pair']} == set(W.PAIR)
    # the launch shapes the large cases are there for: a second grid-stride trip of 128 x 1024 threads, and the 256-block cap
    assert 128 * 1024 < 4099 * 33 <= 1 << 18 < 8195 * 33
    assert all(len(W.shards(c)) == 1 for c in W.WEAK_CASES if c['shape'][0] * c['shape'][1] > 128 * 1024)
    assert any(len(W.shards(c)) == 2 and c['pair'] for c in W.WEAK_CASES) and any(len(W.shards(c)) == 2 and not c['pair'] for c in W.WEAK_CASES)
    for k, vals in W.ADAM_AXES.items():
        assert {c[k] for c in W.ADAM_CASES} == set(vals), k
    assert any(c['lag'] == '3-21' and c['P'] > 21 for c in W.ADAM_CASES) and all(c['extras'] for c in W.ADAM_CASES if c['gsum'] == 'alias')
    assert set(W.ORACLE_SPREAD) <= set(W.BY_ID)
    for cid, spread in W.ORACLE_SPREAD.items():                                  # (re-measured: the reference's own gap)
        assert W.reference(W.BY_ID[cid])['I'].gap() <= spread


# ---- plain-torch stand-ins of the kernels' outputs (to be mutated) ---------------------------------------------------------------------
def standin_weak(c, lo, hi, mutate=None):
    """what one launch of k_weak_partials adds to scal for paths [lo, hi) of the case"""
    o = W.inputs(c)
    N, L, d = c['shape']
    s = slice(lo, hi)
    u, v, vt, f = (o[k][:, s] for k in ('u', 'v', 'vt', 'f'))
    w = o['w'][:, s] if c['weight'] == 'point' else o['w'][s].view(1, -1)
    cN, cNL, ss = W.VOL / N, W.VOL / N / L, o['s3_scale']
    keep = torch.ones(hi - lo, dtype=F64)
    if mutate == 'last_path':
        keep[-1] = 0.0
    phi = v * w
    phit = w * vt + (v * o['wt'][:, s] if o['wt'] is not None else 0.0)
    cl = o['c'][:, s] if o['c'] is not None else W.KAPPA * u
    s3 = cl * u * phi + f * phi
    dphi = o['w0'][s] * o['gxv'][:, s] + v[0] * o['gwx0T'][:, s]
    du = o['gx'][:, s] + o['gs'][s] * o['ghT'][:, s]
    I = torch.zeros(L, hi - lo, dtype=F64)
    if c['grad'] == 's3x':
        s3x = torch.einsum('ijn,in,jn->n', o['a0'][:, :, s], dphi, du)
        if o['b0'] is not None:
            s3x = s3x + v[0] * o['w0'][s] * (o['b0'][:, s] * du).sum(0)
        s3 = s3.clone()
        s3[0] += s3x
    else:
        prod = dphi * du
        if mutate == 'one_trip':
            prod = prod[:min(L, d)]                                              # (i = l only: the stride loop stops after one trip)
        I[0] += cNL * ss * prod.sum(0)
    I[0] -= cN * o['h'][s] * v[0]
    if mutate != 'drop_last_row':
        I[L - 1] += cN * u[L - 1] * v[L - 1]
    out = torch.zeros(16, dtype=F64)
    if c['pair']:
        I += cNL * ss * s3
        out[7], out[8] = (u * keep).sum(), (phit * keep).sum()
    else:
        I -= cNL * (u * phit - ss * s3)
    hr = o['href'][s] if o['href'] is not None else o['h'][s]
    out[0], out[1], out[2] = (I * keep).sum(), (v * v * keep).sum(), ((u[0] - hr) ** 2 * keep).sum()
    return out


def standin_scal(c, mutate=None, stage='sums'):
    o = W.inputs(c)
    N, L, d = c['shape']
    scal = torch.zeros(16, dtype=F64)
    for lo, hi in W.shards(c):
        scal += standin_weak(c, lo, hi, mutate)
    if o['ub'] is not None:
        scal[3] = ((o['ub'] - o['gb']) ** 2).sum()
    if stage == 'final':
        Lb, Nb = o['ub'].shape if o['ub'] is not None else (1, 1)
        if c['pair']:
            scal[0] -= W.VOL / N * scal[7] * scal[8]
            scal[7] = scal[8] = 0.0
        in_ = torch.log(scal[0] ** 2) - torch.log(W.VOL * scal[1] / (N * L))
        scal[6], scal[5] = in_, -in_
        scal[4] = in_ + W.ALPHA * ((scal[2] / N + o['init_off']) + (scal[3] / (Nb * Lb) + o['bdry_off']))
    return scal


def standin_cotangents(c):
    o = W.inputs(c)
    r = W.reference(c)
    N, L, d = c['shape']
    u, v, f = o['u'], o['v'], o['f']
    w = o['w'] if c['weight'] == 'point' else o['w'].view(1, -1)
    cN, cNL, pol = W.VOL / N, W.VOL / N / L, c['pollution']
    cl = o['c'] if o['c'] is not None else W.KAPPA * u
    dI = cNL * o['s3_scale'] * (cl * u + f) * w
    dI[L - 1] += cN * u[L - 1]
    dI[0] -= cN * o['h']
    out = dict(vbar=pol * w - (2.0 / r['I'].value) * dI + 2.0 * v / r['S'].value)
    if not c['pair']:
        dcu = o['c'] + u * o['cp'] if o['c'] is not None else 2.0 * W.KAPPA * u
        B = cNL * dcu * v * w
        B[L - 1] += cN * v[L - 1]
        A = torch.full((L, N), pol, dtype=F64)
        A[0] += W.ALPHA * 2.0 * (u[0] - o['h']) / N
        out.update(ubarA=A, ubarB=B, merged=A + (2.0 / r['I_gen']) * B)
    return out


def standin_adam(c, mutate=None):
    """(param, m, v, g, before) after every update of the case's sequence"""
    r = W.adam_reference(c)
    lo, hi = W.lag_range(c)
    P = c['P']
    p, m, v = r['p0'].clone(), torch.zeros(P, dtype=F64), torch.zeros(P, dtype=F64)
    step = lag = 0
    idx = torch.arange(P)
    lagged = (idx >= lo) & (idx < hi)
    out = []
    for up in r['updates']:
        before = (p.clone(), m.clone(), v.clone())
        g = up['g']
        live = ~(lagged & bool(up['skip']))
        if mutate == 'skip_stepped':
            live = torch.ones(P, dtype=torch.bool)
        t = (step + 1 - lag * lagged.to(F64)).clamp(min=1.0)
        b1 = 0.999 if mutate == 'm_beta2' else 0.9
        mn = b1 * m + (1 - b1) * g
        vn = 0.999 * v + 0.001 * g * g
        pn = p - (W.LR / (1 - 0.9 ** t)) * (mn / (vn.sqrt() / (1 - 0.999 ** t).sqrt() + 1e-8))
        p, m, v = torch.where(live, pn, p), torch.where(live, mn, m), torch.where(live, vn, v)
        step += 1
        lag += 1 if up['skip'] else 0
        out.append((p.clone(), m.clone(), v.clone(), g, before))
    return out


# ---- the stand-ins pass as they are ... --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', W.WEAK_CASES, ids=W.wid)
def test_standin_passes_the_comparison(c):
    W.check_weak_scal(c, standin_scal(c), 'sums')
    if c['final'] != 'none':
        W.check_weak_scal(c, standin_scal(c, stage='final'), 'final')
    r = W.reference(c)
    for k, got in standin_cotangents(c).items():
        for rows in (slice(0, 1), slice(1, None)):
            W.close(got[rows], r[k][rows], W.TOL_ELEM, k)


@pytest.mark.parametrize('c', [c for c in W.WEAK_CASES if c['pair']], ids=W.wid)
def test_pairwise_factorisation_against_the_shaped_oracle(c):
    """s3_scale = Nglob, f := mean f, href := mean h, init_off = var h (and the boundary mean likewise): the O(N) form the caller
    prepares equals the oracle's [N, N] tables"""
    o, r = W.inputs(c), W.reference(c)
    N = c['shape'][0]
    assert torch.equal(o['f'], torch.full_like(o['f'], float(o['f_nat'].mean())))
    scal = standin_scal(c, stage='final')
    assert abs(float(scal[0]) - r['I'].exact) <= W.TOL_REF * r['I'].sum_abs
    h, u0 = o['h'], o['u'][0]
    pairs = torch.mean((u0 - h.unsqueeze(1)) ** 2)                               # src/loss.py:79 on [N] against [N,1], as R.group_forward
    fact = torch.mean((u0 - h.mean()) ** 2) + h.var(unbiased=False)
    assert abs(float(pairs - fact)) <= 1e-13 * float(pairs)
    if c['href']:
        assert o['init_off'] == float(h.var(unbiased=False)) and torch.equal(o['href'], torch.full((N,), float(h.mean()), dtype=F64))
    g = torch.Generator().manual_seed(5)
    ub_s, gcol = torch.randn(N, 1, generator=g, dtype=F64), torch.randn(N, 1, generator=g, dtype=F64)
    pairs_b = torch.mean((ub_s - gcol.unsqueeze(2)) ** 2)                        # src/loss.py:84: [n,1] - [n,1,1] -> [n,n,1]
    fact_b = torch.mean((ub_s - gcol.mean()) ** 2) + gcol.var(unbiased=False)
    assert abs(float(pairs_b - fact_b)) <= 1e-13 * float(pairs_b)


@pytest.mark.parametrize('c', W.ADAM_CASES, ids=W.aid)
def test_adam_standin_passes_the_comparison(c):
    for it, (p, m, v, g, before) in enumerate(standin_adam(c)):
        W.check_adam(c, it, p, m, v, gsum=g, before=before)


# ---- ... and fail under each mutation ----------------------------------------------------------------------------------------------------
def _case(shape, pair=False, **want):
    return next(c for c in W.WEAK_CASES if c['shape'] == shape and c['pair'] == pair and all(c[k] == v for k, v in want.items()))


MUTATIONS = [('drop_last_row', c) for c in (_case((1, 1, 1)), _case((5, 3, 7)), _case((8195, 33, 4)), _case((37, 1, 5), True))]
MUTATIONS += [('one_trip', c) for c in W.WEAK_CASES if c['regime'] == 'L<d' and c['grad'] == 'inline']
MUTATIONS += [('last_path', c) for c in (_case((5, 3, 7)), _case((4099, 33, 4)), _case((8195, 33, 4)), _case((1100, 1, 3), True))]
assert any(m == 'one_trip' for m, _ in MUTATIONS)


@pytest.mark.parametrize('mutate,c', MUTATIONS, ids=lambda x: x if isinstance(x, str) else W.wid(x))
def test_a_mutated_reduction_fails_the_comparison(mutate, c):
    with pytest.raises(AssertionError):
        W.check_weak_scal(c, standin_scal(c, mutate), 'sums')


@pytest.mark.parametrize('c', [_case((8195, 33, 4)), _case((5, 3, 7)), _case((37, 1, 5), True)], ids=W.wid)
def test_an_unwritten_cotangent_entry_fails(c):
    r = W.reference(c)
    L, N = c['shape'][1], c['shape'][0]
    for k, got in standin_cotangents(c).items():
        got[L - 1, N - 1] = float('nan')
        with pytest.raises(AssertionError):
            W.close(got[L - 1:], r[k][L - 1:], W.TOL_ELEM, k)


def _fails(c, seq):
    try:
        for it, (p, m, v, g, before) in enumerate(seq):
            W.check_adam(c, it, p, m, v, gsum=g, before=before)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('c', W.ADAM_CASES, ids=W.aid)
def test_adam_mutations_fail(c):
    assert _fails(c, standin_adam(c, 'm_beta2')) or all(float(up['g'].abs().max()) == 0.0 for up in W.adam_reference(c)['updates'])
    if c['lag'] != 'empty':
        assert _fails(c, standin_adam(c, 'skip_stepped'))


def test_an_overwritten_guard_is_reported_on_the_cpu():
    arena = G.Arena('cpu', chunk=1 << 14)
    scal = arena.out(16, name='scal')
    work = arena.out(6 * 1024 + 8, name='work')
    work.zero_()
    scal[:9] = 0.0
    arena.check(written=[scal[:9]], untouched=[scal[9:]])
    base = work.data_ptr()
    raw = next(ch for ch in arena.chunks if ch.raw.data_ptr() <= base < ch.raw.data_ptr() + 8 * ch.raw.numel())
    e = (base - raw.raw.data_ptr()) // 8 + work.numel()                          # the first double behind xw_reduce_work_size()
    raw.f64[e] = 0.0
    with pytest.raises(AssertionError, match='guard band overwritten'):
        arena.check()
    raw.raw[e] = G.PATTERN
    scal[12] = 1.0
    with pytest.raises(AssertionError, match='untouched'):
        arena.check(untouched=[scal[9:]])
