"""Every compiled kernel of the fused stepper against the oracle: the 90 cases of tests/stepper_inventory.py -- every container of
kernels.ODE_WIDTHS x depth 1..10 x euler, midpoint, rk4 -- each with every launch form that exists for it (FORMS: six forward forms,
nine sweeps), so that every instantiation of k_ode_fwd, n4::k_ode_fwd_n4, k_ode_bwd, k_ode_bwd_duo and n4::k_ode_bwd_n4 runs under a
test (tests/test_stepper_inventory_host.py: the forms reach exactly the kernels the library holds).

One shape for all cases, N = 17 paths, L = 3 times, d = 3: two 16-path tiles, the second with one live path (tile indexing, lane
masking); two steps (a first and a later step of the sweep, two slots of the activation store).  The forms are inside a case, so the
oracle runs once per case.

Reference: the oracle's autograd (tests/test_gpu_edges._fused_oracle, _grads, _check_params); for the adjoint forms the oracle with
adjoint=True (oracle/refspec.py's restatement of odeint_adjoint, as tests/test_gpu_kernels.test_ode_backward_continuous_adjoint), gx
exactly zero.  No kernel is compared with another.  _close's metric at the project's tolerances: u, Y 1e-12; gx, gs, every
parameter's gradient and their sum 1e-10.  At (64, 16, 10) tests/test_gpu_edges.py's rule applies: ORACLE_SPREAD holds the oracle's
own rounding spread (hidden units permuted, paths reversed; CPU), and a tolerance is 8 x the spread where that exceeds an eighth of
it -- it does not, the project's tolerances stand.  `python tests/test_gpu_stepper_inventory.py` prints the table (CPU only).

Guards: every operand is a view of a guarded.Arena, outputs, slabs and stores start as the NaN pattern, and check() demands u, Y, gx,
gs and the slabs written.  The activation store [step][tile of 16 paths][row][16], from csrc/xw_ode_fwd.h and xw_ode_core.h (k_ode_fwd, act_store):
  full store (16-path forward)     every double row is written in all three containers.  K rows of a layer are whole 4-row blocks
                                   plus, at (20, 10), one partial block of K mod 4 = 2 rows whose 32 doubles the lane groups 0 and 1
                                   fill (ActLane.off_part_st; groups 2 and 3 carry an out-of-range offset); K mod 4 = 0 at (32, 12)
                                   and (64, 16).  The stage inputs are whole blocks (H mod 4 = 0).  Padding paths of the last tile
                                   store copies into slots of their own.
  x-only store (16-path forward)   the tanh rows of every stage are written; the layer-input rows and the stage-input rows are left
                                   untouched (SinkAct<K, M, false>::z stores nothing, the stage inputs are stored under ACT == 1 only)
  mask-word rows, narrow stores    the 2 x words rows per stage behind the doubles hold 32-bit mask words, and the narrow-tile
                                   forward (csrc/xw_ode_n4.h) has store code of its own: guard bands only
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import guarded as G  # noqa: E402
import stepper_inventory as SI  # noqa: E402
from test_gpu_edges import (DEVICE, TOL_GRAD, TOL_VALUE, _check_params, _fused_oracle, _grads, _oracle, _permuted,  # noqa: E402
                            _unpermuted)
from test_gpu_tiled_stepper import U_ORDER, _close  # noqa: E402

pytestmark = pytest.mark.gpu

N, L, D = 17, 3, 3
SEED0 = 2000                                        # case i is seeded 2000 + 10 i


def _cid(c):
    return '%dx%d-m%d-%s' % c


# The oracle's own rounding spread at the widest, deepest corner (oracle_spreads below; float64, CPU; _close's metric):
# (u and Y, gradients of the discrete oracle, gradients of the adjoint oracle).  Every other case: the project's tolerances.
ORACLE_SPREAD = {
    (64, 16, 10, 'euler'): (4.84e-16, 9.63e-16, 2.67e-15),
    (64, 16, 10, 'midpoint'): (3.45e-16, 1.20e-15, 2.49e-15),
    (64, 16, 10, 'rk4'): (4.97e-16, 1.69e-15, 9.94e-16),
}
assert set(ORACLE_SPREAD) == {c for c in SI.CASES if c[:3] == (64, 16, 10)}


def _tolerances(c):
    """(u and Y, discrete gradients, adjoint gradients): the project's, or 8 x the oracle's spread where that exceeds an eighth"""
    sv, sg, sa = ORACLE_SPREAD.get(c, (0.0, 0.0, 0.0))
    return tuple(8 * s if s > tol / 8 else tol for s, tol in ((sv, TOL_VALUE), (sg, TOL_GRAD), (sa, TOL_GRAD)))


def _adjoint_oracle(theta, m, solver, x, t, start):
    """the oracle with adjoint=True: u [N, L] (attached) and the leaves (x, start, the parameters in U_ORDER)"""
    from oracle import refspec as R
    th = {k: v.clone().requires_grad_(True) for k, v in theta.items()}
    x64, s = x.clone().requires_grad_(True), start.clone().requires_grad_(True)
    n, l, d = x.shape[0], t.shape[0], x.shape[1]
    X = torch.cat((t.view(1, l, 1).expand(n, l, 1), x64.view(n, 1, d).expand(n, l, d)), 2)
    u = R.u_net(th, {'u_layers': m, 'solver': solver, 'adjoint': True}, X, s)
    return u, [x64, s] + [th[k] for k in U_ORDER]


def _store_regions(act, tiles, H, K, m, stages, x_only):
    """(written, untouched) of a 16-path forward's activation store, as (tensor, mask) entries of Arena.check"""
    rec = act.view(act.shape[0], tiles, act.shape[1], 16)
    doubles = stages * m * K + (stages - 1) * H     # ActLayout::ROWS: the mask-word rows lie behind them
    row = torch.arange(act.shape[1])
    tanh = torch.zeros_like(row, dtype=torch.bool)
    for i in range(stages):
        tanh |= (row >= i * m * K + (m - 1) * K) & (row < (i + 1) * m * K)
    full = lambda mask: mask.view(1, 1, -1, 1).expand(rec.shape)                            # noqa: E731
    if x_only:
        return [(rec, full(tanh))], [(rec, full((row < doubles) & ~tanh))]
    return [(rec, full(row < doubles))], []


def _run(c, n, l, d, seed, forms, switch_sets=({},)):
    """every form of `forms` at case c on n paths, l times: launches in one arena, guards, then the comparisons -- once per entry of
    `switch_sets` (library switches, the arguments of kernels.switched), every time against the same oracle"""
    from xnode_wan_pde_solver_amd import kernels as KN
    oracle = _fused_oracle(c[0], c[1], c[2], d, n, l, c[3], seed)
    adjoint = []                                    # (the adjoint oracle's gradients, once a form asks for them)
    for sw in switch_sets:
        with KN.switched(**sw):
            _run_once(KN, c, n, l, d, forms, oracle, adjoint)


def _run_once(KN, c, n, l, d, forms, oracle, adjoint):
    H, K, m, method = c
    assert KN.stepper_family(H, K, m) == 'mfma'
    tol_v, tol_g, tol_a = _tolerances(c)
    theta, blob, x, t, start, ubar, u_ref, Y_ref, leaves = oracle
    mid = KN.method_id(method)
    rows, cols, P = KN.ode_act_rows(mid, H, K, m), KN.ode_act_cols(n), blob.numel()
    stages = {'euler': 1, 'midpoint': 2, 'rk4': 4}[method]
    arena = G.Arena(torch.device(DEVICE))
    tc, bc = arena.inp(t, name='t'), arena.inp(blob, name='theta')
    xT, st, ub = arena.inp(x.t(), name='xT'), arena.inp(start, name='start'), arena.inp(ubar.t(), name='ubar')
    fwd, sweeps, written, untouched = {}, {}, [], []
    for f in forms:
        if f in SI.FWD_FORMS:
            spec = SI.FWD_FORMS[f]
            job = dict(xT=xT, start=st, u=arena.out(l, n, name=f + '.u'), Y=arena.out(l, H, n, name=f + '.Y'))
            if spec['store'] is not None:
                job['act'] = arena.out(l - 1, rows, cols, name=f + '.act')
            KN.ode_fwd_multi([job], tc, bc, mid, H, K, m, act_x_only=spec['store'] == 'x', narrow=spec['narrow'])
            fwd[f] = job
            written += [job['u'], job['Y']]
            if spec['store'] is not None and not spec['narrow']:
                w_, u_ = _store_regions(job['act'], cols // 16, H, K, m, stages, spec['store'] == 'x')
                written += w_
                untouched += u_
    for f in forms:
        if f in SI.BWD_FORMS:
            spec = SI.BWD_FORMS[f]
            j = dict(fwd[spec['producer']], ubar=ub, gx=arena.out(d, n, name=f + '.gx'), gs=arena.out(n, name=f + '.gs'))
            if spec['params']:
                j['gslab'] = arena.out(KN.ode_bwd_slabs(n), P, name=f + '.gslab')
            KN.ode_bwd_multi([j], tc, bc, mid, H, K, m, want_x=True, want_params=spec['params'], adjoint=spec['adjoint'],
                             narrow=spec['narrow'])
            sweeps[f] = j
            written += [j['gx'], j['gs']] + ([j['gslab']] if spec['params'] else [])
    arena.check(written=written, untouched=untouched)
    for f, job in fwd.items():
        _close(job['u'].t(), u_ref.detach(), tol_v, f + ' u')
        _close(job['Y'], Y_ref, tol_v, f + ' Y')
    want = _grads(u_ref, leaves, ubar)
    for f, j in sweeps.items():
        if SI.BWD_FORMS[f]['adjoint']:
            if not adjoint:
                u_adj, leaves_adj = _adjoint_oracle(theta, m, method, x, t, start)
                adjoint.append(_grads(u_adj, leaves_adj, ubar))
                assert float(adjoint[0][0].abs().max()) == 0.0      # x is not an input of odeint_adjoint
            assert float(j['gx'].abs().max()) == 0.0, f + ' gx'
            w, tol = adjoint[0], tol_a
        else:
            _close(j['gx'].t(), want[0], tol_g, f + ' gx')
            w, tol = want, tol_g
        _close(j['gs'], w[1], tol, f + ' gs')
        if 'gslab' in j:
            _check_params(KN.slab_sum(j['gslab']).cpu(), theta, w, tol, f)


@pytest.mark.parametrize('c', SI.CASES, ids=_cid)
def test_every_form_against_the_oracle(c):
    _run(c, N, L, D, SEED0 + 10 * SI.CASES.index(c), SI.forms_of(*c))


def test_duo_sweep_spacer_round():
    """the duo sweep's spacer round (xw_ode_select.h duo_grid: spread, tiles in (ncu, 2 ncu], i.e. above 4096 paths on this
    chip): every second round of blocks ends at once and the tile index is folded back.  One tile more than the chip has CUs, with
    the library switch duo_spread on (the default, read back from the library) and once more with it off: one block per tile.  The
    launcher's own count of CUs the test mirrors but cannot observe; the result is compared with the oracle either way."""
    from xnode_wan_pde_solver_amd import kernels as KN
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert KN.switches()['duo_spread'] is True
    n = 16 * (ncu + 1)
    assert ncu < (n + 15) // 16 <= 2 * ncu
    _run((20, 10, 8, 'midpoint'), n, 2, D, SEED0 - 1, ['fwd_store', 'duo'], switch_sets=({}, dict(duo_spread=False)))


# ---- the oracle's own rounding spread (CPU) ------------------------------------------------------------------------------------------
def oracle_spreads(c):
    """(u and Y, discrete gradients, adjoint gradients) of one case in _close's metric: the oracle as written against the oracle with
    the hidden units of both widths permuted and the paths in reverse order"""
    H, K, m, method = c
    seed = SEED0 + 10 * SI.CASES.index(c)
    theta, _, x, t, start, ubar, u, Y, leaves = _fused_oracle(H, K, m, D, N, L, method, seed)
    tp, ph, pk = _permuted(theta, D, H, K, seed + 3000)
    inv_h, inv_k = torch.argsort(ph), torch.argsort(pk)
    rev = torch.arange(N - 1, -1, -1)
    xr, sr, ur = x[rev].contiguous(), start[rev].contiguous(), ubar[rev].contiguous()

    def rel(a, b):
        return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)

    def grad_spread(g, g2):
        back = [_unpermuted(k, a, D, inv_h, inv_k) for k, a in zip(U_ORDER, g2[2:])]
        pairs = [(g2[0][rev], g[0]), (g2[1][rev], g[1])] + list(zip(back, g[2:]))
        pairs.append((torch.cat([a.reshape(-1) for a in back]), torch.cat([b.reshape(-1) for b in g[2:]])))
        return max(rel(a, b) for a, b in pairs)

    u2, Y2, leaves2 = _oracle(tp, m, method, xr, t, sr)
    sv = max(rel(u2.detach()[rev], u.detach()), rel(Y2[:, inv_h][:, :, rev], Y))
    sg = grad_spread(_grads(u, leaves, ubar), _grads(u2, leaves2, ur))
    ua, la = _adjoint_oracle(theta, m, method, x, t, start)
    ua2, la2 = _adjoint_oracle(tp, m, method, xr, t, sr)
    return sv, sg, grad_spread(_grads(ua, la, ubar), _grads(ua2, la2, ur))


if __name__ == '__main__':
    print('| case | u, Y | discrete gradients | adjoint gradients | tolerances |')
    for c_ in SI.CASES:
        if c_ in ORACLE_SPREAD or '--all' in sys.argv:
            print('| %s | %.2e | %.2e | %.2e | %s |' % ((_cid(c_),) + oracle_spreads(c_) + (_tolerances(c_),)))
