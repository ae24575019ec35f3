"""Every compiled test-network kernel against the oracle, inside a guarded arena: the cases of tests/testnet_inventory.py -- one per
instantiation of k_disc_fwd, k_disc_rec and k_disc_bwd (csrc/xw_disc_fwd.hip, xw_disc_rec.hip, xw_disc_bwd.hip) at the smallest shape that selects it, k_disc_xproj, the
tiled family's kernel per row-tile count, the generic pair at five widths, and the edges of the selection rules (d = 24 | 25,
52 | 53, 46 | 47, 94 | 95, 62 | 63, 126).  tests/test_testnet_inventory_host.py: the cases reach exactly the kernels the library holds.

Every operand a case hands to kernels.py is a view of one guarded.Arena: xT, t / tpp, phi, vbar and (as an input of the forward) the
x-projection table; v, vt, gxv, gtv, the record, the slabs and the table (as the output of disc_xproj) start as the NaN pattern.
What the case does NOT hand over is outside the guards: where no recomputing kernel exists, kernels.disc_gradx allocates the
forward's v, and kernels.disc_bwd without a record allocates the record it stores first, with torch.empty (the 'gradx' cases and
the 'bwd' cases without a record away from W = 50, q = 9: 11 of the 123) -- their inputs and results are guarded, those two buffers
are not, and cannot be without a change to kernels.py; the same kernels run fully guarded in the 'fwd' and record cases.  After one
synchronize Arena.check demands (from the kernels' code):
  written     v; vt unless want_vt=False; gxv / gtv of a launch with ngrad > 0 ([d, ngrad] and [ngrad]: the gradient's last tile is
              ragged); every slab row kernels.disc_bwd_slabs promises; the table, padding rows included; the record: ALL of it at the
              MFMA containers (tile-major, and every lane of the ragged last tile stores a copy of the last valid point into a slot of
              its own -- k_disc_fwd's record stores are not masked by pt.valid, and k_disc_rec reads those columns with cotangent
              zero, so they must be finite), the valid points' columns in the tiled family (tile-major) and on the generic path
              (row-major)
  untouched   gxv / gtv of a launch without gradient and vt under want_vt=False (not handed to the kernel); the record's columns
              past the last point in the tiled family and on the generic path (only valid points store)

Reference: oracle/refspec.py's v_net and its autograd in float64 (tests/test_gpu_edges._testnet_reference_nl), never another kernel.
Compared in _close's metric: v (TOL_VALUE 1e-12); vt, gxv, gtv (TOL_TANGENT 1e-11); the phi gradient per parameter block and as a
whole (TOL_GRAD 1e-10); the table against x Vin[:, 1:]^T + Vin.b (TOL_VALUE) with its padding rows exactly zero.  ORACLE_SPREAD holds
the oracle's own rounding spread at the corners (W = 128, q = 16, d = 126; the deepest generic case) -- the oracle as written against
the oracle with the hidden units permuted and the points reversed, CPU -- and a tolerance is 8 x the spread where that exceeds an
eighth of it; it does not: the project's tolerances stand.  `python tests/test_gpu_testnet_inventory.py --spread` prints the table
(CPU only).

The kernels behind disc_vin_lds off (k_disc_fwd<50 | 64, *, *, 0>) and the rotated first round of the static split behind
disc_dynamic off run in this process like every other case: run_case issues a case's launches inside kernels.switched(...) with the
library switches the case is described with (options.EngineOptions; the library reads them at each launch call).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import guarded as G  # noqa: E402
import testnet_inventory as TI  # noqa: E402
from test_gpu_edges import DEVICE, TOL_GRAD, TOL_TANGENT, TOL_VALUE, V_ORDER, _testnet_reference_nl  # noqa: E402
from test_gpu_tiled_stepper import _close  # noqa: E402

pytestmark = pytest.mark.gpu

SEED0 = 4000                                        # case i of TI.CASES is seeded 4000 + 10 i


def _seed(c):
    return SEED0 + 10 * TI.CASES.index(c) if c in TI.CASES else SEED0 - 10


# The oracle's own rounding spread at the corners (oracle_spread below; float64, CPU; _close's metric): (v; vt, gxv, gtv; the phi
# gradient per block and whole), per case id.  Every other case: the project's tolerances.
ORACLE_SPREAD = {
    'fwd-mfma-W128-q16-d126-path17x1-rec-ngrad17': (2.71e-15, 2.73e-15, 1.89e-15),
    'bwd-mfma-W128-q16-d126-path128x3-rec-ngrad64': (1.20e-14, 2.13e-15, 2.50e-15),
    'bwd-mfma-W128-q16-d126-point17x1-rec': (1.25e-15, 2.46e-15, 1.30e-15),
    'bwd-mfma-W127-q16-d1-path17x1-rec-ngrad17': (6.21e-16, 4.50e-15, 2.56e-15),
    'gradx-mfma-W128-q16-d126-point15x1': (1.97e-15, 5.25e-15, 1.64e-15),
}                                                   # (every spread is below an eighth of its tolerance: the project's stand)


def _corner(c):
    """the widest, deepest container shape at the widest input, and the deepest generic case"""
    return (c.W, c.q, c.d) == (128, 16, 126) or (c.family == 'mfma' and c.W == 127 and c.q == 16)


def _tolerances(c):
    """(v, tangents, gradients): the project's, or 8 x the oracle's spread where that exceeds an eighth"""
    spread = ORACLE_SPREAD.get(TI.cid(c), (0.0, 0.0, 0.0))
    return tuple(8 * s if s > tol / 8 else tol for s, tol in zip(spread, (TOL_VALUE, TOL_TANGENT, TOL_GRAD)))


# ---- a case: reference, operands, launches, checks -----------------------------------------------------------------------------------
def reference(c):
    """the host values of a case's inputs and the oracle's results: v [P] and the input gradient [P, d + 1] in the kernels' point
    order (time-major), the phi gradient of <vbar, v>"""
    phi, x, t, tpp, vbar, N, L, v_ref, gX, gphi = _testnet_reference_nl(c.W, c.q, c.d, c.mode, c.N, c.L, _seed(c))
    if c.mode == 'path':
        v_ref, gX, vb = v_ref.t().reshape(-1), gX.permute(1, 0, 2).reshape(N * L, c.d + 1), vbar.t().contiguous()
    else:
        vb = vbar.view(1, N)
    return dict(phi=phi, x=x, t=t, tpp=tpp, vbar=vb, v=v_ref, gX=gX, gphi=gphi)


def operands(arena, c, ref):
    """every operand of the case as a view of `arena`"""
    from xnode_wan_pde_solver_amd import kernels as KN
    N, L, d = c.N, c.L, c.d
    ops = dict(xT=arena.inp(ref['x'].t(), name='xT'), phi=arena.inp(torch.cat([ref['phi'][k].reshape(-1) for k in V_ORDER]), name='phi'),
               t=arena.inp(ref['t'], name='t') if ref['t'] is not None else None,
               tpp=arena.inp(ref['tpp'], name='tpp') if ref['tpp'] is not None else None,
               vbar=arena.inp(ref['vbar'], name='vbar'))
    if c.entry == 'gradx':
        ops.update(gxv=arena.out(d, N, name='gxv'), gtv=arena.out(N, name='gtv'))
        return ops
    if c.entry == 'fwd' or c.record:
        ops.update(v=arena.out(L, N, name='v'), vt=arena.out(L, N, name='vt'))
        ops.update(gxv=arena.out(d, c.ngrad or N, name='gxv'), gtv=arena.out(c.ngrad or N, name='gtv'))
        if c.xproj:
            ops['xproj'] = arena.out(KN.disc_xproj_rows(c.W), N, name='xproj')
        if c.record:
            ops['act'] = arena.out(KN.disc_act_rows(c.W, c.q, c.family), KN.disc_act_cols(N * L), name='act')
    if c.entry == 'bwd':
        ops['gslab'] = arena.out(KN.disc_bwd_slabs(N, L), ops['phi'].numel(), name='gslab')
    return ops


def launches(c, ops):
    """the case's calls of kernels.disc_xproj / disc_fwd / disc_bwd / disc_gradx"""
    from xnode_wan_pde_solver_amd import kernels as KN
    now = KN.switches()                             # the library stands at the switches the case is described with
    for attr, field in TI.SWITCHES.items():
        assert now[field] == getattr(c, attr), (TI.ENV[field], now[field])
    if c.entry == 'gradx':
        KN.disc_gradx(ops['xT'], ops['t'], ops['phi'], c.W, c.q, tpp=ops['tpp'], vbar=ops['vbar'], gxv=ops['gxv'], gtv=ops['gtv'],
                      family=c.family)
        return
    if 'v' in ops:
        if c.xproj:
            KN.disc_xproj(ops['xT'], ops['phi'], c.W, out=ops['xproj'])
        grad = dict(gxv=ops['gxv'], gtv=ops['gtv'], ngrad=c.ngrad) if c.ngrad else {}
        KN.disc_fwd(ops['xT'], ops['t'], ops['phi'], c.W, c.q, tpp=ops['tpp'], want_vt=c.want_vt, v=ops['v'], vt=ops['vt'],
                    max_blocks=c.max_blocks, act=ops.get('act'), xproj=ops.get('xproj'), family=c.family, **grad)
    if c.entry == 'bwd':
        KN.disc_bwd(ops['xT'], ops['t'], ops['phi'], ops['vbar'], c.W, c.q, tpp=ops['tpp'], gslab=ops['gslab'], act=ops.get('act'),
                    family=c.family)


def _record_regions(c, act):
    """(written, untouched) of the record, as entries of Arena.check"""
    rows, cols, P = act.shape[0], act.shape[1], c.N * c.L
    if c.family == 'mfma' and c.W in TI.CONTAINERS:
        return [act], []                            # every lane of the last tile has a slot (k_disc_fwd)
    if c.family == 'tiled':                         # [tiles of 16 points][rows][16]
        rec = act.view(cols // 16, rows, 16)
        point = (torch.arange(cols // 16).view(-1, 1, 1) * 16 + torch.arange(16).view(1, 1, 16)).expand(cols // 16, rows, 16)
    else:                                           # the generic path: [rows][columns]
        rec, point = act, torch.arange(cols).view(1, -1).expand(rows, cols)
    return [(rec, point < P)], [(rec, point >= P)]


def verify(arena, c, ops, ref):
    """guards, written and untouched regions, then every result against the oracle.  Works on whatever device the arena is on: the
    host test hands it CPU tensors standing in for device output."""
    tol_v, tol_t, tol_g = _tolerances(c)
    N, L, d, gX = c.N, c.L, c.d, ref['gX']
    if c.entry == 'gradx':
        arena.check(written=[ops['gxv'], ops['gtv']])
        w = ref['vbar'].reshape(-1, 1)
        _close(ops['gxv'].t(), gX[:, 1:] * w, tol_t, 'nabla_x <vbar, v>')
        _close(ops['gtv'], gX[:, 0] * w[:, 0], tol_t, 'd/dt <vbar, v>')
        return
    written, untouched = [], []
    if 'v' in ops:
        written.append(ops['v'])
        (written if c.want_vt else untouched).append(ops['vt'])
        (written if c.ngrad else untouched).extend([ops['gxv'], ops['gtv']])
        if c.xproj:
            written.append(ops['xproj'])
        if c.record:
            w_, u_ = _record_regions(c, ops['act'])
            written += w_
            untouched += u_
    if c.entry == 'bwd':
        written.append(ops['gslab'])
    arena.check(written=written, untouched=untouched)
    if 'v' in ops:
        _close(ops['v'].reshape(-1), ref['v'], tol_v, 'v')
        if c.want_vt:
            _close(ops['vt'].reshape(-1), gX[:, 0], tol_t, 'dv/dt')
        if c.ngrad:
            _close(ops['gxv'].t(), gX[:c.ngrad, 1:], tol_t, 'nabla_x v at the leading points')
            _close(ops['gtv'], gX[:c.ngrad, 0], tol_t, 'dv/dt (reverse) at the leading points')
        if c.xproj:
            phi = ref['phi']
            _close(ops['xproj'][:c.W].t(), ref['x'] @ phi['Vin'][:, 1:].t() + phi['Vin_b'], tol_v, 'x projection')
            assert float(ops['xproj'][c.W:].abs().sum()) == 0.0, 'padding rows of the x projection'
    if c.entry == 'bwd':
        flat, off = ops['gslab'].detach().cpu().sum(0), 0
        for k in V_ORDER:
            n = ref['phi'][k].numel()
            _close(flat[off:off + n], ref['gphi'][off:off + n], tol_g, 'phi gradient ' + k)
            off += n
        assert off == flat.numel()
        _close(flat, ref['gphi'], tol_g, 'phi gradient')


def run_case(c, device=DEVICE):
    from xnode_wan_pde_solver_amd import kernels as KN
    assert KN.testnet_family(c.W, c.q) in KN.TESTNET_FAMILIES           # (a served shape)
    ref = reference(c)
    arena = G.Arena(torch.device(device))
    ops = operands(arena, c, ref)
    with KN.switched(**TI.switched_off(c)):         # (read on the host when a launch is called: the block need not outlast the kernels)
        launches(c, ops)
    verify(arena, c, ops, ref)


# 111 cases at the defaults, 8 behind disc_vin_lds off, 4 behind disc_dynamic off
BEHIND = {field: [c for c in TI.CASES if TI.switched_off(c) == {field: False}] for field in ('disc_vin_lds', 'disc_dynamic')}
assert sum(TI.in_process(c) for c in TI.CASES) == 111 and {f: len(v) for f, v in BEHIND.items()} == {'disc_vin_lds': 8, 'disc_dynamic': 4}
assert 111 + 8 + 4 == len(TI.CASES)
assert {TI.cid(c) for c in TI.CASES if _corner(c)} == set(ORACLE_SPREAD)


@pytest.mark.parametrize('c', TI.CASES, ids=TI.cid)
def test_case_against_the_oracle_under_guards(c):
    assert not _corner(c) or TI.cid(c) in ORACLE_SPREAD
    run_case(c)


def test_depth_17_with_the_fused_gradient_is_refused():
    """the launch of the q = 17 case, with gxv: the ReLU-mask stash of k_disc_fwd holds 16 layers"""
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    c = next(c for c in TI.CASES if c.q == 17 and c.family == 'mfma')
    assert c.W == 50 and c.ngrad == 0 and ('fwd', 50, True, False, 6) in TI.reaches(c)
    ref = reference(c)
    arena = G.Arena(torch.device(DEVICE))
    ops = operands(arena, c, ref)
    with pytest.raises(XnwanError):
        KN.disc_fwd(ops['xT'], ops['t'], ops['phi'], c.W, c.q, v=ops['v'], vt=ops['vt'], gxv=ops['gxv'], gtv=ops['gtv'], ngrad=c.N,
                    act=ops['act'], family='mfma')
    arena.check(untouched=[ops['v'], ops['vt'], ops['gxv'], ops['gtv'], ops['act']])


# ---- the oracle's own rounding spread (CPU) ------------------------------------------------------------------------------------------
def oracle_spread(c):
    """(v; tangents; gradients) of one case in _close's metric: the oracle as written against the oracle with the hidden units
    permuted and the points in reverse order (the same mathematics in another summation order)"""
    from oracle import refspec as R
    phi, x, t, tpp, vbar, N, L, v, gX, gphi = _testnet_reference_nl(c.W, c.q, c.d, c.mode, c.N, c.L, _seed(c))
    X = (torch.cat((t.view(1, L, 1).expand(N, L, 1), x.view(N, 1, c.d).expand(N, L, c.d)), 2) if c.mode == 'path'
         else torch.cat((tpp.view(N, 1), x), 1))
    p = torch.randperm(c.W, generator=torch.Generator().manual_seed(_seed(c) + 3))
    inv = torch.argsort(p)
    ph = {'Vin': phi['Vin'][p], 'Vin_b': phi['Vin_b'][p], 'Vh': phi['Vh'][p][:, p], 'Vh_b': phi['Vh_b'][p], 'Vo': phi['Vo'][:, p],
          'Vo_b': phi['Vo_b']}
    ph = {k: a.clone().contiguous().requires_grad_(True) for k, a in ph.items()}
    flip = (lambda a: a.flip(0, 1)) if c.mode == 'path' else (lambda a: a.flip(0))
    X2 = flip(X).contiguous().requires_grad_(True)
    v2 = R.v_net(ph, {'v_layers': c.q}, X2)
    used = [k for k in V_ORDER if c.q > 0 or not k.startswith('Vh')]
    g2 = dict(zip(used, torch.autograd.grad((v2 * flip(vbar)).sum(), [ph[k] for k in used], retain_graph=True)))
    gX2 = flip(torch.autograd.grad(v2.sum(), X2)[0])
    back = {'Vin': lambda a: a[inv], 'Vin_b': lambda a: a[inv], 'Vh': lambda a: a[inv][:, inv], 'Vh_b': lambda a: a[inv],
            'Vo': lambda a: a[:, inv], 'Vo_b': lambda a: a}
    blocks = [(back[k](g2[k]) if k in g2 else torch.zeros_like(phi[k])).reshape(-1) for k in V_ORDER]

    def rel(a, b):
        return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)

    sg, off = rel(torch.cat(blocks), gphi), 0
    for b in blocks:
        sg = max(sg, rel(b, gphi[off:off + b.numel()]))
        off += b.numel()
    return rel(flip(v2.detach()), v), max(rel(gX2[..., 0], gX[..., 0]), rel(gX2[..., 1:], gX[..., 1:])), sg


if __name__ == '__main__' and '--spread' in sys.argv:
    print('| case | v | vt, gxv, gtv | phi gradient | tolerances |')
    for c_ in TI.CASES:
        if _corner(c_) or '--all' in sys.argv:
            print('| %s | %.2e | %.2e | %.2e | %s |' % ((TI.cid(c_),) + oracle_spread(c_) + (_tolerances(c_),)))
