"""Edge shapes and several jobs per launch of the per-path evaluation kernels inside the guard-banded, poisoned arena of
tests/guarded.py: the five fixed-grid kernels behind evaluate / evaluate_grad / evaluate_hvp / evaluate_quad / evaluate_vjp
(csrc/xw_tiled_paths.hip, _grad.hip, _hvp.hip, _jet.hip, _vjp.hip) and the dopri5 pair (csrc/xw_tdopri_paths.hip, _grad.hip).

1. Edge shapes (test_per_path_kernels_at_edge_shapes).  One case is one shape and runs all five fixed-grid kernels on the inputs of
   tests/test_gpu_eval_paths._ragged (a path without a step beside one with L - 1 in one tile, a start time per path).  The cases
   are a seeded covering selection (tests/test_gpu_edges.cover) over N, H, K, m, the named (H, K, m) of that file, d, L and the
   jet's R: every value of every axis occurs with every method; the module asserts its own coverage when it is collected.  Per case
     * every operand comes from one Arena, the hvp / jet / vjp workspaces through work=; Arena.check: no guard element touched,
       every element of u, Y, gx, gs, ut, gslab, ju, hx, hs, Yd, quu written; theta and every input keep their bits;
     * every path against oracle.refspec run on that path ALONE (the _oracle_alone of tests/test_gpu_eval_paths / _grad / _hess /
       _vjp: autograd, double backward), never against another kernel, in _close's metric: 1e-12 on u, Y; 1e-10 on gx, gs, ut, ju,
       hx, hs, Yd, quu and on each parameter block of slab_sum(gslab) (tests/test_gpu_eval_vjp._check_blocks, its exact-zero rules
       for m == 1 and L == 1 included);
     * the jet's u has the forward's bits, its ju those of the hvp launch on direction 0; a path without a step has gx == 0,
       hx == 0 and hs == 0 exactly;
     * no compared reference is identically zero unless it is so by construction (L == 1: no step anywhere, so gx, hx, hs and the
       bare curvature vanish): asserted, never skipped.  The seed of a case (theta, inputs, directions, weights) comes from CASE_SEED,
       chosen on the CPU from SEED_LIST as the first under which this holds -- at H = 1 the lift's single ReLU is closed on every
       path under many seeds.
   Tolerances at the corners -- (256, 256, 32), H = 1 with K = 256, every m >= 31 -- follow tests/test_gpu_edges.py's rule from
   ORACLE_SPREAD below: the oracle as written against the oracle with the hidden units permuted and the paths reversed, per output
   group (values, first order, second order, parameter gradients); 8 x the spread where it exceeds an eighth of the project
   tolerance, the project tolerance elsewhere.  `python tests/test_gpu_paths_edges.py` prints the cases, their seeds, every
   reference scale and the table on the CPU (profiles/r31_paths_edges.md keeps it).

2. Several jobs in one launch (test_several_jobs_in_one_launch, test_dopri5_several_jobs_in_one_launch): the per-job workspace
   offsets of all eight entry points.  Four jobs of N = 1, 16, 17, 33 paths with inputs of their own, optional pointers varied per
   job (nstep on two of them; a grad job asking ut alone; a vjp job without gx, gs; an hvp job asking ju alone; a jet job without
   qs and u; the jet's R = 1, 3, 2, 1), one guarded workspace per launch: every output of every job -- for dopri5 the int32 status,
   n_acc and n_att too -- has the bits of the same job launched alone (a path's bits do not depend on its neighbours: no oracle, no
   step-decision conditioning needed), the guards are whole, the inputs unchanged.  At (17, 17, 2) every job's outputs are compared
   with the oracle as in part 1 as well: the bits compared are right, not merely equal."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import guarded as G  # noqa: E402
from test_gpu_tiled_stepper import F64, U_ORDER, _close, _theta  # noqa: E402
from test_gpu_edges import D_MAX, NAMED, _check_d_max, _permuted, _unpermuted, cover, missing  # noqa: E402
from test_gpu_eval_paths import METHODS, _ragged, _oracle_alone as _oracle_fwd  # noqa: E402
from test_gpu_eval_grad import _oracle_alone as _oracle_grad  # noqa: E402
from test_gpu_eval_hess import _oracle_alone as _oracle_hess  # noqa: E402
from test_gpu_eval_quad import _curves  # noqa: E402  (direction 0 of its curves: test_gpu_eval_hess._directions)
from test_gpu_eval_vjp import _blocks, _check_blocks, _weights, _oracle_alone as _oracle_vjp  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_V, TOL_G = 1e-12, 1e-10                           # u, Y; every derivative and every parameter block
GROUPS = ('values', 'first', 'second', 'params')
GROUP_TOL = {'values': TOL_V, 'first': TOL_G, 'second': TOL_G, 'params': TOL_G}
GROUP_OF = {'u': 'values', 'Y': 'values', 'gx': 'first', 'gs': 'first', 'ut': 'first', 'ju': 'first', 'Yd': 'first',
            'hx': 'second', 'hs': 'second', 'quu': 'second'}
SPREAD_MAX = 1e-11                                    # a case whose oracle spreads further takes another seed, not a wider bound

# ---- 1. the covering selection --------------------------------------------------------------------------------------------------------
AXES = {
    'N': (1, 2, 15, 16, 17, 31, 32, 33, 47),
    'H': (1, 3, 4, 15, 16, 17, 65, 255, 256),
    'K': (1, 3, 4, 15, 16, 17, 65, 255, 256),
    'm': (1, 2, 31, 32),
    'named': NAMED + (None,),                         # one of the named (H, K, m), or None: H, K, m drawn on their own
    'd': (1, 2, D_MAX),
    'L': (1, 2, 5),
    'R': (1, 3),                                      # the jet's directions
}
PARTNERS = {'method': METHODS}
SEED_LIST = tuple(range(500, 508))


def _named(rnd, c):
    if c['named'] is not None:
        c['H'], c['K'], c['m'] = c['named']


def _cid(c):
    return '%s-N%d-H%dK%dm%d-d%d-L%d-R%d' % (c['method'], c['N'], c['H'], c['K'], c['m'], c['d'], c['L'], c['R'])


# The seed of every case that does not take SEED_LIST[0]: the first of SEED_LIST under which no compared reference is identically
# zero (chosen by choose_seed below, on the CPU; `python tests/test_gpu_paths_edges.py` prints the choice and every scale)
CASE_SEED = {
    'midpoint-N17-H1K1m1-d126-L1-R3': 502,
    'rk4-N1-H1K1m1-d1-L5-R1': 504,
    'euler-N1-H1K1m1-d2-L5-R1': 502,
    'rk4-N16-H1K256m3-d126-L5-R1': 501,
    'euler-N16-H1K256m3-d1-L5-R1': 501,
}


def _cases():
    # (the selection's seed: of 0 .. 39, the covering selection whose most expensive host reference -- paths x steps x stages x
    # layers x launches -- is the cheapest; it keeps (256, 256, 32) over two tiles at d = 126 and m >= 31 over L = 5)
    cases = cover(AXES, PARTNERS, fixed=_named, seed=16)
    for c in cases:
        c['seed'] = CASE_SEED.get(_cid(c), SEED_LIST[0])
    return cases


CASES = _cases()
assert not missing(CASES, AXES, PARTNERS), missing(CASES, AXES, PARTNERS)
assert 30 <= len(CASES) <= 60, len(CASES)
assert len({_cid(c) for c in CASES}) == len(CASES) and all(k in {_cid(c) for c in CASES} for k in CASE_SEED)


def _corner(c):
    return (c['H'], c['K'], c['m']) == (256, 256, 32) or (c['H'], c['K']) == (1, 256) or c['m'] >= 31


# The oracle's own rounding spread at the corners (oracle_spread below, float64, CPU), per case id and output group
# (values: u, Y; first order: gx, gs, ut, ju, Yd; second order: hx, hs, quu; parameter gradients: the blocks of the weighted sum)
ORACLE_SPREAD = {
    'rk4-N31-H256K256m32-d126-L2-R1': (9.16e-16, 2.83e-15, 5.92e-15, 1.02e-14),
    'euler-N2-H256K256m32-d126-L2-R3': (3.84e-16, 3.45e-15, 2.57e-14, 3.44e-15),
    'midpoint-N1-H256K16m32-d2-L5-R3': (2.63e-16, 6.65e-16, 1.37e-15, 1.18e-15),
    'euler-N31-H16K16m31-d1-L5-R1': (2.26e-16, 1.14e-15, 5.15e-16, 1.17e-15),
    'rk4-N32-H65K65m31-d1-L1-R1': (2.66e-16, 8.18e-16, 8.51e-16, 6.81e-16),
    'midpoint-N33-H65K4m31-d126-L2-R1': (3.56e-16, 8.96e-16, 9.55e-14, 2.09e-15),
    'euler-N32-H3K65m31-d2-L2-R1': (2.57e-16, 1.75e-15, 1.93e-15, 2.96e-15),
    'midpoint-N47-H1K256m3-d2-L1-R3': (0.00e+00, 2.58e-15, 0.00e+00, 9.77e-16),
    'euler-N47-H15K4m32-d126-L1-R1': (1.17e-16, 5.81e-16, 1.23e-16, 5.27e-16),
    'rk4-N15-H3K3m32-d126-L1-R3': (1.59e-16, 7.49e-16, 2.91e-16, 4.06e-16),
    'euler-N15-H4K256m32-d2-L5-R1': (6.12e-16, 4.62e-15, 2.95e-15, 1.77e-15),
    'midpoint-N16-H256K256m32-d2-L2-R1': (3.68e-16, 1.03e-13, 4.54e-15, 1.59e-13),
    'midpoint-N32-H16K3m32-d2-L1-R1': (2.70e-16, 6.76e-15, 3.90e-16, 4.16e-16),
    'rk4-N16-H1K256m3-d126-L5-R1': (7.82e-17, 6.17e-16, 5.87e-16, 4.37e-16),
    'euler-N16-H1K256m3-d1-L5-R1': (2.55e-16, 1.02e-15, 7.00e-16, 1.39e-15),
}                                                     # (every spread is far below an eighth of its tolerance: the project's stand)

if __name__ != '__main__':                            # (run as a script, the module prints the table it would hold)
    assert all(_cid(c) in ORACLE_SPREAD for c in CASES if _corner(c)) and all(any(_cid(c) == k for c in CASES) for k in ORACLE_SPREAD)
    assert all(s <= SPREAD_MAX for v in ORACLE_SPREAD.values() for s in v)


def _tolerances(c):
    """group -> tolerance: the project's, or 8 x the oracle's measured spread where that exceeds an eighth of it"""
    spread = ORACLE_SPREAD.get(_cid(c), (0.0,) * len(GROUPS))
    return {g: (8 * s if s > GROUP_TOL[g] / 8 else GROUP_TOL[g]) for g, s in zip(GROUPS, spread)}


# ---- the inputs and the oracle of one group of paths -------------------------------------------------------------------------------------
def _inputs(N, L, d, R, seed):
    """the host side of one group: _ragged's paths, R curves (direction 0: _directions(N, d, seed + 2)) and the weights"""
    x, start, n, tT = _ragged(N, L, d, seed + 1000)
    vx, vs, qs = _curves(N, d, R, seed + 2000)
    assert float(qs.abs().min()) > 0
    return dict(x=x, start=start, n=n, tT=tT, vx=vx, vs=vs, qs=qs, w=_weights(N, seed + 3000))


def _reference(theta, H, K, m, method, inp, key):
    """every compared output of one group from the oracle, every path ALONE: dict(u [L, N], Y, gx, gs, ut, ju [R, N], hx, hs, Yd
    (direction 0), quu [R, N], bare [R, N] -- quu without its qs term --, gflat -- the weighted sum of the paths' parameter
    gradients --, wgx, wgs).  The oracles keep what they computed under `key`"""
    x, start, n, tT, vx, vs, qs, w = (inp[k] for k in ('x', 'start', 'n', 'tT', 'vx', 'vs', 'qs', 'w'))
    (N, d), R = x.shape, vx.shape[0]
    ref = {}
    ref['u'], ref['Y'] = _oracle_fwd(theta, H, K, m, method, x, start, n, tT, key)
    ref['gx'], ref['gs'], ref['ut'] = _oracle_grad(theta, H, K, m, method, x, start, n, tT, key)
    ref['ju'], ref['quu'], ref['bare'] = (torch.empty(R, N, dtype=F64) for _ in range(3))
    for r in range(R):
        ju, hx, hs, Yd, gs = _oracle_hess(theta, H, K, m, method, x, start, n, tT, vx[r], vs[r], key + ('direction', r))
        ref['ju'][r], ref['bare'][r] = ju, (vx[r].t() * hx).sum(0) + vs[r] * hs
        ref['quu'][r] = ref['bare'][r] + gs * qs[r]
        if r == 0:
            ref['hx'], ref['hs'], ref['Yd'] = hx, hs, Yd
    Gm, gx, gs = _oracle_vjp(theta, H, K, m, method, x, start, n, tT, key)
    ref['gflat'], ref['wgx'], ref['wgs'] = (w.view(-1, 1) * Gm).sum(0), w.view(1, -1) * gx, w * gs
    return ref


def _forget(key):
    """drops what the four oracles keep under `key` (one test uses it; the widest cases hold a gradient per path and parameter)"""
    for name in ('test_gpu_eval_paths', 'test_gpu_eval_grad', 'test_gpu_eval_hess', 'test_gpu_eval_vjp'):
        kept = sys.modules[name]._ORACLE
        for k in [k for k in kept if k[:len(key)] == key]:
            del kept[k]


def _zero_by_construction(k, L):
    """L == 1: no path takes a step, the lift alone is piecewise linear in the start value and does not see x"""
    return L == 1 and k in ('gx', 'wgx', 'hx', 'hs', 'bare')


def _scales(ref, L):
    """name -> the reference's scale, asserted nonzero unless zero by construction (then asserted zero); the parameter blocks are
    held to the same by _check_blocks"""
    out = {}
    for k, v in ref.items():
        if k == 'gflat':
            continue
        out[k] = float(v.abs().max())
        if _zero_by_construction(k, L):
            assert out[k] == 0.0, k
        else:
            assert out[k] > 0.0, 'a comparison of zeros: ' + k
    return out


# ---- the launches of one group ---------------------------------------------------------------------------------------------------------
FWD_IN = ('xT', 'start', 'tT')


def _place(arena, inp, hint):
    """the group's operands in the arena: the shared inputs (nstep where `hint`), the curves and the weights"""
    dev = dict(xT=arena.inp(inp['x'].t(), name='xT'), start=arena.inp(inp['start'], name='start'), tT=arena.inp(inp['tT'], name='tT'),
               vx=arena.inp(inp['vx'].transpose(1, 2), name='vx'), vs=arena.inp(inp['vs'], name='vs'), qs=arena.inp(inp['qs'], name='qs'),
               w=arena.inp(inp['w'], name='w'))
    if hint:
        dev['nstep'] = inp['n'].to(torch.int32).to(arena.device)
    return dev


def _jobs(arena, dev, L, H, P, want=None):
    """the five jobs of one group on the placed operands `dev`, outputs from the arena.  want: entry -> the optional outputs asked
    for (None: all of them); 'qs' among the jet's stands for the input"""
    d, N = dev['xT'].shape
    R = dev['vx'].shape[0]
    want = want or {}
    base = {k: dev[k] for k in FWD_IN + ('nstep',) if k in dev}
    shape = dict(gx=(d, N), u=(N,), ju=(R, N), quu=(R, N))     # (the jet's u, ju, quu; every other output is [N])
    fwd = dict(base, u=arena.out(L, N, name='u'), Y=arena.out(L, H, N, name='Y'))
    back = dict(base, Y=fwd['Y'])
    grad = dict(back, **{k: arena.out(*shape.get(k, (N,)), name=k) for k in want.get('grad', ('gx', 'gs', 'ut'))})
    vjp = dict(back, w=dev['w'], gslab=arena.out((N + 15) // 16, P, name='gslab'),
               **{k: arena.out(*shape.get(k, (N,)), name='w' + k) for k in want.get('vjp', ('gx', 'gs'))})
    hvp = dict(back, vx=dev['vx'][0], vs=dev['vs'][0], Yd=arena.out(L, H, N, name='Yd'),
               **{k: arena.out(*((d, N) if k == 'hx' else (N,)), name=k) for k in want.get('hvp', ('ju', 'hx', 'hs'))})
    jw = want.get('jet', ('u', 'ju', 'quu', 'qs'))
    jet = dict(base, vx=dev['vx'], vs=dev['vs'], **{k: arena.out(*shape[k], name='jet.' + k) for k in jw if k != 'qs'})
    if 'qs' in jw:
        jet['qs'] = dev['qs']
    return dict(fwd=fwd, grad=grad, vjp=vjp, hvp=hvp, jet=jet)


ENTRY_OUTS = dict(fwd=('u', 'Y'), grad=('gx', 'gs', 'ut'), vjp=('gslab', 'gx', 'gs'), hvp=('ju', 'hx', 'hs', 'Yd'), jet=('u', 'ju', 'quu'))


def _launch(KN, arena, groups, blob, mid, d, H, K, m):
    """the five entry points, one launch each over the jobs of `groups` (a list of _jobs results), the forward first; the vjp, hvp
    and jet workspaces guarded views handed in through work= (the forward's and the sweep's: Arena.workspaces), returned with their
    block counts"""
    tiles = sum((g['fwd']['xT'].shape[1] + 15) // 16 for g in groups)
    blocks = sum(g['jet']['vx'].shape[0] * ((g['jet']['xT'].shape[1] + 15) // 16) for g in groups)
    KN.tiled_paths_fwd([g['fwd'] for g in groups], blob, mid, H, K, m)
    KN.tiled_paths_grad([g['grad'] for g in groups], blob, mid, H, K, m)
    works = [(arena.out(KN.lib.xw_paths_tiled_vjp_work(d, H, K, m) * tiles, name='vjp_work'), tiles),
             (arena.out(KN.lib.xw_paths_tiled_hvp_work(d, H, K, m) * tiles, name='hvp_work'), tiles),
             (arena.out(KN.lib.xw_paths_tiled_jet_work(d, H, K, m) * blocks, name='jet_work'), blocks)]
    KN.tiled_paths_vjp([g['vjp'] for g in groups], blob, mid, H, K, m, work=works[0][0])
    KN.tiled_paths_hvp([g['hvp'] for g in groups], blob, mid, H, K, m, work=works[1][0])
    KN.tiled_paths_jet([g['jet'] for g in groups], blob, mid, H, K, m, work=works[2][0])
    return works


def _every_block_used(works, what):
    """every block's share of a handed-in workspace holds something a kernel stored: a per-job offset that advances too little
    leaves the last shares the poison they started with (one that advances too much ends in a guard band, Arena.check's finding)"""
    for i, (work, blocks) in enumerate(works):
        used = (work.view(blocks, -1).view(torch.int64) != G.PATTERN).any(1)
        assert bool(used.all()), '%s: the workspace share of block %d of launch %d (vjp, hvp, jet) was never written' % (
            what, int(torch.nonzero(~used)[0]), i)


def _written(groups):
    return [g[e][k] for g in groups for e, outs in ENTRY_OUTS.items() for k in outs if k in g[e]]


def _compare(KN, g, ref, inp, blocks, m, L, tol, what, record=None):
    """the outputs one group's jobs hold against the oracle's `ref`, in _close's metric; every error is printed (and kept in
    `record`: group -> largest) before it is asserted"""
    record = {} if record is None else record

    def held(label, a, b, grp):
        scale = float(b.abs().max())
        err = float((a.cpu() - b).abs().max()) / max(scale, 1e-300)
        print('%s %s: rel-to-scale error %.3e (scale %.3e)' % (label, what, err, scale))
        record[grp] = max(record.get(grp, 0.0), err)
        _close(a, b, tol[grp], '%s %s' % (label, what))

    for k in ('u', 'Y'):
        held(k, g['fwd'][k], ref[k], GROUP_OF[k])
    for k in ('gx', 'gs', 'ut'):
        if k in g['grad']:
            held(k, g['grad'][k], ref[k], GROUP_OF[k])
    for k in ('ju', 'hx', 'hs', 'Yd'):
        if k in g['hvp']:
            held(k, g['hvp'][k], ref['ju'][0] if k == 'ju' else ref[k], GROUP_OF[k])
    jet = g['jet']
    if 'ju' in jet:
        held('jet ju', jet['ju'], ref['ju'], 'first')
    if 'quu' in jet:                                                # (without qs: the curvature alone)
        held('jet quu', jet['quu'], ref['quu'] if 'qs' in jet else ref['bare'], 'second')
    for k in ('gx', 'gs'):
        if k in g['vjp']:
            held('vjp ' + k, g['vjp'][k], ref['w' + k], 'first')
    worst = {}
    try:
        assert tol['params'] == TOL_G                              # (_check_blocks holds its own bound: the project's)
        _check_blocks(KN.slab_sum(g['vjp']['gslab']), ref['gflat'], blocks, m, L, what, worst)
    finally:
        record['params'] = max(record.get('params', 0.0), max(worst.values(), default=0.0))
        print('parameter blocks %s: largest rel-to-scale error %.3e' % (what, record['params']))


def _identities(g, inp, dev_, what):
    """what costs no reference: the jet's u and ju are the forward's and the hvp's; no step, no x gradient and no curvature"""
    L = g['fwd']['u'].shape[0]
    still = (inp['n'] == 0).to(dev_)
    if 'u' in g['jet']:
        assert torch.equal(g['jet']['u'], g['fwd']['u'][L - 1]), 'the jet\'s u has the forward\'s bits: ' + what
    if 'ju' in g['jet'] and 'ju' in g['hvp']:
        assert torch.equal(g['jet']['ju'][0], g['hvp']['ju']), 'the jet\'s ju on direction 0 has the hvp\'s bits: ' + what
    for e, k in (('grad', 'gx'), ('vjp', 'gx'), ('hvp', 'hx')):
        if k in g[e]:
            assert bool((g[e][k][:, still] == 0).all()), '%s of a path without a step: %s' % (k, what)
    if 'hs' in g['hvp']:
        assert bool((g['hvp']['hs'][still] == 0).all()), 'hs of a path without a step: ' + what


def _keep(tensors):
    return [(t, t.clone()) for t in tensors]


def _unchanged(kept, what):
    for i, (t, c) in enumerate(kept):
        assert torch.equal(t.view(torch.int64) if t.dtype == F64 else t, c.view(torch.int64) if c.dtype == F64 else c), \
            'input %d changed: %s' % (i, what)


@pytest.mark.parametrize('c', CASES, ids=_cid)
def test_per_path_kernels_at_edge_shapes(c):
    from xnode_wan_pde_solver_amd import kernels as KN
    method, N, H, K, m, d, L, R, seed = (c[k] for k in ('method', 'N', 'H', 'K', 'm', 'd', 'L', 'R', 'seed'))
    assert KN.stepper_family(H, K, m, 'generic', KN.method_id(method)) in ('tiled', 'mfma')     # (a served shape)
    _check_d_max()
    what = _cid(c)
    theta, blob_h = _theta(H, K, m, d, seed)
    inp = _inputs(N, L, d, R, seed)
    if L == 5 and N > 1:
        assert int(inp['n'][0]) == 0 and int(inp['n'][1]) == 4       # no step beside four, in one tile
    dev = torch.device('cuda')
    mid = KN.method_id(method)
    arena = G.Arena(dev)
    with arena.workspaces(KN):
        blob = arena.inp(blob_h, name='theta')
        placed = _place(arena, inp, hint=CASES.index(c) % 2 == 0)
        torch.cuda.synchronize()
        kept = _keep([blob] + list(placed.values()))
        g = _jobs(arena, placed, L, H, blob.numel())
        works = _launch(KN, arena, [g], blob, mid, d, H, K, m)
    arena.check(written=_written([g]))
    _every_block_used(works, what)
    _unchanged(kept, what)
    ref = _reference(theta, H, K, m, method, inp, ('paths_edges', what))
    _forget(('paths_edges', what))
    print('reference scales %s: %s' % (what, ', '.join('%s %.2e' % kv for kv in _scales(ref, L).items())))
    record = {}
    try:
        _compare(KN, g, ref, inp, _blocks(theta, d), m, L, _tolerances(c), what, record)
    finally:
        print('largest device error %s: %s' % (what, ', '.join('%s %.2e' % (k, record[k]) for k in GROUPS if k in record)))
    _identities(g, inp, dev, what)


# ---- 2. several jobs in one launch ------------------------------------------------------------------------------------------------------
JOB_SIZES = (1, 16, 17, 33)
JOB_R = (1, 3, 2, 1)                                  # the jet's directions per job: its workspace offset advances by R tiles
JOB_HINT = (True, False, True, False)                 # nstep on two of the jobs
JOB_WANT = ({}, dict(grad=('ut',), jet=('ju', 'quu')), dict(vjp=()), dict(hvp=('ju',)))   # job 1's jet: no u, no qs
MULTI_SHAPES = ((17, 17, 2, 2), (65, 15, 3, 1), (256, 255, 1, 5))                        # (H, K, m, d)
MULTI_L = 5


@pytest.mark.parametrize('shape', range(len(MULTI_SHAPES)))
@pytest.mark.parametrize('method', METHODS)
def test_several_jobs_in_one_launch(method, shape):
    from xnode_wan_pde_solver_amd import kernels as KN
    H, K, m, d = MULTI_SHAPES[shape]
    L, dev, mid = MULTI_L, torch.device('cuda'), KN.method_id(method)
    theta, blob_h = _theta(H, K, m, d, 41 + shape)
    inps = [_inputs(N, L, d, R, 700 + 10 * shape + i) for i, (N, R) in enumerate(zip(JOB_SIZES, JOB_R))]
    arena = G.Arena(dev)
    with arena.workspaces(KN):
        blob = arena.inp(blob_h, name='theta')
        placed = [_place(arena, inp, hint) for inp, hint in zip(inps, JOB_HINT)]
        torch.cuda.synchronize()
        kept = _keep([blob] + [t for p in placed for t in p.values()])
        together = [_jobs(arena, p, L, H, blob.numel(), w) for p, w in zip(placed, JOB_WANT)]
        works = _launch(KN, arena, together, blob, mid, d, H, K, m)
        alone = [_jobs(arena, p, L, H, blob.numel(), w) for p, w in zip(placed, JOB_WANT)]
        for g in alone:
            _launch(KN, arena, [g], blob, mid, d, H, K, m)
    arena.check(written=_written(together) + _written(alone))
    _every_block_used(works, '%s %s' % (method, MULTI_SHAPES[shape]))
    _unchanged(kept, '%s %s' % (method, MULTI_SHAPES[shape]))
    for i, (a, b) in enumerate(zip(together, alone)):
        for e, outs in ENTRY_OUTS.items():
            for k in outs:
                assert (k in a[e]) == (k in b[e])
                if k in a[e]:
                    assert torch.equal(a[e][k], b[e][k]), '%s of job %d (%s): not the bits of the job alone' % (k, i, e)
    assert 'u' not in together[1]['jet'] and 'qs' not in together[1]['jet'] and set(ENTRY_OUTS['grad']) & set(together[1]['grad']) == {'ut'}
    assert 'gx' not in together[2]['vjp'] and set(ENTRY_OUTS['hvp']) & set(together[3]['hvp']) == {'ju', 'Yd'}
    if shape == 0:                                                   # ... and the bits are the right ones
        tol = dict(GROUP_TOL)
        for i, (g, inp) in enumerate(zip(together, inps)):
            what = '%s %s job %d' % (method, MULTI_SHAPES[shape], i)
            ref = _reference(theta, H, K, m, method, inp, ('paths_edges several jobs', method, i))
            _scales(ref, L)
            _compare(KN, g, ref, inp, _blocks(theta, d), m, L, tol, what)
            _identities(g, inp, dev, what)


# dopri5: the forward with and without its checkpoint form and the sweep, at two networks of tests/test_gpu_eval_dopri5.py with its
# paths; job i takes the N_i paths from offset JOB_FIRST[i] on (inputs of its own)
JOB_FIRST = (3, 7, 11, 4)
DOPRI_NETS = (0, 3)
I32, I64 = torch.int32, torch.int64


def _dopri_job(arena, x, start, t_in, t_end, H, cap, ckpt, rec=True, fin=True):
    N = x.shape[0]
    ints = {k: arena.out((N + 1) // 2, name=k).view(I32) for k in ('status', 'n_acc', 'n_att')}
    job = dict(xT=arena.inp(x.t(), name='xT'), start=arena.inp(start, name='start'), t_in=arena.inp(t_in, name='t_in'),
               t_end=arena.inp(t_end, name='t_end'), u=arena.out(N, name='u'), Y=arena.out(H, N, name='Y'), ints=ints,
               **{k: v[:N] for k, v in ints.items()})
    if rec:
        job['rec'] = arena.out(cap, 2, N, name='rec')
    if fin:
        job['fin'] = arena.out(2, N, name='fin')
    if ckpt:
        job['ckpt'] = arena.out(cap, H, N, name='ckpt')
    return job


def _dopri_sweep_job(arena, fj, want):
    d, N = fj['xT'].shape
    job = {k: fj[k] for k in ('xT', 'start', 't_in', 't_end', 'n_acc', 'rec', 'ckpt', 'Y')}
    job.update({k: arena.out(*((d, N) if k == 'gx' else (N,)), name=k) for k in want})
    return job


def _same_bits(a, b, keys, what):
    for k in keys:
        assert (k in a) == (k in b)
        if k in a:
            va, vb = (a[k].view(I64), b[k].view(I64)) if a[k].dtype == F64 else (a[k], b[k])      # (NaN poison compares as bits)
            assert torch.equal(va, vb), '%s: %s is not the bits of the job alone' % (what, k)


@pytest.mark.parametrize('net', DOPRI_NETS)
def test_dopri5_several_jobs_in_one_launch(net):
    import test_gpu_eval_dopri5 as E
    from test_gpu_eval_grad_dopri5 import _check_forwards
    from xnode_wan_pde_solver_amd import kernels as KN
    d, H, K, m = E.NETS[net]
    dev = torch.device('cuda')
    _, blob_h = _theta(H, K, m, d, 500 + net)
    x, start, t_in, t_end, _ = E._paths(d, E.SEEDS[net])
    cut = [slice(f, f + N) for f, N in zip(JOB_FIRST, JOB_SIZES)]
    assert all(s.stop <= E.NMAX for s in cut)
    sweep_want = (('gx', 'gs', 'ut'), ('ut',), ('gx', 'gs'), ('gs',))
    arena = G.Arena(dev)

    def forward_jobs(ckpt):                                          # (without ckpt: job 1 without rec and fin as well)
        return [_dopri_job(arena, x[s], start[s], t_in[s], t_end[s], H, E.CAP, ckpt, rec=ckpt or i != 1, fin=ckpt or i != 1)
                for i, s in enumerate(cut)]

    with arena.workspaces(KN):
        blob = arena.inp(blob_h, name='theta')
        plain, kept_f = forward_jobs(False), forward_jobs(True)
        plain_1, kept_1 = forward_jobs(False), forward_jobs(True)
        torch.cuda.synchronize()
        kept = _keep([blob] + [j[k] for js in (plain, kept_f, plain_1, kept_1) for j in js for k in ('xT', 'start', 't_in', 't_end')])
        KN.paths_dopri5_fwd(plain, blob, H, K, m, H)
        KN.paths_dopri5_fwd(kept_f, blob, H, K, m, H)
        for j in plain_1 + kept_1:
            KN.paths_dopri5_fwd([j], blob, H, K, m, H)
        sweeps = [_dopri_sweep_job(arena, fj, w) for fj, w in zip(kept_f, sweep_want)]
        sweeps_1 = [_dopri_sweep_job(arena, fj, w) for fj, w in zip(kept_1, sweep_want)]
        KN.paths_dopri5_grad(sweeps, blob, H, K, m)
        for j in sweeps_1:
            KN.paths_dopri5_grad([j], blob, H, K, m)
    _check_forwards(arena, plain + kept_f + plain_1 + kept_1, written=[j[k] for j in sweeps + sweeps_1 for k in ('gx', 'gs', 'ut') if k in j])
    _unchanged(kept, 'dopri5 net %d' % net)
    for i in range(len(cut)):
        assert int((kept_f[i]['status'] != 0).sum()) == 0 and int(kept_f[i]['n_acc'].max()) <= E.CAP     # (the sweep's premise)
        fwd_keys = ('u', 'Y', 'fin', 'rec', 'ckpt', 'status', 'n_acc', 'n_att')
        _same_bits(plain[i], plain_1[i], fwd_keys, 'forward, job %d' % i)
        _same_bits(kept_f[i], kept_1[i], fwd_keys, 'forward with checkpoints, job %d' % i)
        _same_bits(plain[i], kept_f[i], ('u', 'Y', 'status', 'n_acc', 'n_att'), 'with and without checkpoints, job %d' % i)
        _same_bits(sweeps[i], sweeps_1[i], ('gx', 'gs', 'ut'), 'sweep, job %d' % i)
    assert int(max(j['n_acc'].max() for j in kept_f)) > 1           # (steps were taken: the records are not empty)


# ---- the CPU side: seeds, scales and the oracle's own spread -----------------------------------------------------------------------------
def _case_reference(c, seed, tag):
    method, N, H, K, m, d, L, R = (c[k] for k in ('method', 'N', 'H', 'K', 'm', 'd', 'L', 'R'))
    theta, _ = _theta(H, K, m, d, seed)
    inp = _inputs(N, L, d, R, seed)
    ref = _reference(theta, H, K, m, method, inp, (tag, _cid(c), seed))
    _forget((tag, _cid(c), seed))
    return theta, inp, ref


def _block_scales(c, theta, ref):
    """the scale of every parameter block of the weighted sum, with _check_blocks's by-construction zeros left out"""
    out = {}
    for name, idx in _blocks(theta, c['d']).items():
        field = name in ('Wh', 'Wh_b', 'Wo', 'Wo_b', 'Win_b') or name.startswith('Win')
        if not ((c['m'] == 1 and name in ('Wh', 'Wh_b')) or (c['L'] == 1 and field)):
            out[name] = float(ref['gflat'][idx].abs().max())
    return out


def choose_seed(c):
    """(seed, scales): the first seed of SEED_LIST under which no compared reference of the case is identically zero"""
    for seed in SEED_LIST:
        theta, inp, ref = _case_reference(c, seed, 'choose')
        try:
            scales = _scales(ref, c['L'])
        except AssertionError:
            continue
        scales.update(_block_scales(c, theta, ref))
        if min(v for k, v in scales.items() if not _zero_by_construction(k, c['L'])) > 0:
            return seed, scales
    raise AssertionError('no seed of SEED_LIST serves %s' % _cid(c))


def oracle_spread(c):
    """per output group, the spread of one case in _close's metric: the oracle as written against the oracle with the hidden units
    of both widths permuted and the paths in reverse order (the same mathematics in another summation order)"""
    method, N, H, K, m, d, L, R = (c[k] for k in ('method', 'N', 'H', 'K', 'm', 'd', 'L', 'R'))
    theta, inp, ref = _case_reference(c, c['seed'], 'choose')
    tp, ph, pk = _permuted(theta, d, H, K, c['seed'] + 3000)
    inv_h, inv_k = torch.argsort(ph), torch.argsort(pk)
    rev = torch.arange(N - 1, -1, -1)
    inp2 = dict(x=inp['x'][rev].contiguous(), start=inp['start'][rev].contiguous(), n=inp['n'][rev].contiguous(),
                tT=inp['tT'][:, rev].contiguous(), vx=inp['vx'][:, rev].contiguous(), vs=inp['vs'][:, rev].contiguous(),
                qs=inp['qs'][:, rev].contiguous(), w=inp['w'][rev].contiguous())
    ref2 = _reference(tp, H, K, m, method, inp2, ('spread', _cid(c), c['seed']))
    _forget(('spread', _cid(c), c['seed']))
    back = {k: v[..., rev] for k, v in ref2.items() if k != 'gflat'}
    back['Y'], back['Yd'] = back['Y'][:, inv_h], back['Yd'][:, inv_h]
    parts, off = [], 0
    for k in U_ORDER:                                                # the summed gradient, back in the original order of the units
        n_ = tp[k].numel()
        parts.append(_unpermuted(k, ref2['gflat'][off:off + n_].view(tp[k].shape), d, inv_h, inv_k).reshape(-1))
        off += n_
    back['gflat'] = torch.cat(parts)

    def rel(a, b):
        return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)

    out = {g: 0.0 for g in GROUPS}
    for k, grp in list(GROUP_OF.items()) + [('wgx', 'first'), ('wgs', 'first'), ('bare', 'second')]:
        out[grp] = max(out[grp], rel(back[k], ref[k]))
    for name, idx in _blocks(theta, d).items():
        if float(ref['gflat'][idx].abs().max()) > 0:
            out['params'] = max(out['params'], rel(back['gflat'][idx], ref['gflat'][idx]))
    return tuple(out[g] for g in GROUPS)


if __name__ == '__main__':
    import time
    print('%d cases (+ %d fixed-grid launches of several jobs, %d dopri5)' % (len(CASES), 3 * len(MULTI_SHAPES), len(DOPRI_NETS)))
    print('| case | seed | reference scales | parameter blocks: smallest scale |')
    for c_ in CASES:
        t0_ = time.time()
        seed_, sc_ = choose_seed(c_)
        blocks_ = {k: v for k, v in sc_.items() if k in _blocks(_theta(c_['H'], c_['K'], c_['m'], c_['d'], seed_)[0], c_['d'])}
        print('| %s | %d%s | %s | %.2e | (%.1f s)' % (_cid(c_), seed_, '' if seed_ == c_['seed'] else ' (CASE_SEED holds %d)' % c_['seed'],
                                                    ', '.join('%s %.2e' % (k, v) for k, v in sc_.items() if k not in blocks_),
                                                    min(blocks_.values()), time.time() - t0_), flush=True)
    print('| corner case | values | first order | second order | parameter gradients | tolerances |')
    for c_ in CASES:
        if _corner(c_):
            c_['seed'] = choose_seed(c_)[0]
            s_ = oracle_spread(c_)
            print("    '%s': (%s),   # %s" % (_cid(c_), ', '.join('%.2e' % v for v in s_),
                                             ', '.join('%.0e' % (8 * v if v > GROUP_TOL[g] / 8 else GROUP_TOL[g]) for g, v in zip(GROUPS, s_))),
                  flush=True)
