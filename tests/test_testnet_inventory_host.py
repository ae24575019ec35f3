"""The test network's inventory (tests/testnet_inventory.py) against the built library: every compiled test-network kernel is reached
by a case of tests/test_gpu_testnet_inventory.py, and every case lands on kernels that exist; the comparison helper of that file fails
on a slightly wrong result; its spread table still holds.  CPU only."""
import collections
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402
import testnet_inventory as TI  # noqa: E402


def test_every_compiled_testnet_kernel_is_reached_and_every_case_lands_on_one():
    from xnode_wan_pde_solver_amd import _lib, kernels as KN
    assert tuple(KN.DISC_WIDTHS) == TI.CONTAINERS and KN.DISC_MAX_GRAD_DEPTH == TI.QMAX
    have = TI.compiled(_lib.LIB_PATH)
    want = TI.reached()
    print('compiled test-network kernels: %d; reached: %d by %d cases' % (len(have), len(want), len(TI.CASES)))
    assert not TI.UNREACHED                          # (a table, should reading the dispatch ever prove a kernel unselectable)
    assert not have - set(want) - set(TI.UNREACHED), 'compiled, but no case runs them: %s' % sorted(have - set(want), key=repr)
    assert not set(want) - have, 'forms that land on a kernel the library does not hold: %s' % sorted(
        ((k, [TI.cid(c) for c in want[k]]) for k in set(want) - have), key=repr)
    # what the library holds today (a change detector beside the set equality): 48 / 24 / 4 / 1 of csrc/xw_disc_fwd.hip, _rec, _bwd, 4 + 4 of the
    # tiled family, the generic pair
    assert collections.Counter(k[0] for k in have) == {'fwd': 48, 'rec': 24, 'bwd': 4, 'xproj': 1, 't_fwd': 4, 't_bwd': 4,
                                                       'g_fwd': 1, 'g_bwd': 1}
    fwd = {k for k in have if k[0] == 'fwd'}
    assert fwd == ({('fwd', W, a, dy, v) for W in (50, 64) for a in (False, True) for dy in (False, True) for v in (-1, 0, 6, 13)}
                   | {('fwd', W, a, dy, v) for W in (96, 128) for a in (False, True) for dy in (False, True) for v in (-1, 0)})
    assert {k for k in have if k[0] == 'rec'} == {('rec', W, 0, ng, ts) for W in TI.CONTAINERS for ng in (1, 2, 3) for ts in (False, True)}
    assert {k for k in have if k[0] == 'bwd'} == {('bwd', 50, 9, ctg, p, not p) for ctg in (1, 2) for p in (False, True)}
    assert {k[1] for k in have if k[0] == 't_fwd'} == {k[1] for k in have if k[0] == 't_bwd'} == {4, 8, 12, 16}
    # all instantiations of one container kernel sit in one code object (what else a translation unit holds moves code generation)
    objs = TI.code_objects(_lib.LIB_PATH)
    for family in ('fwd', 'rec', 'bwd'):
        assert sum(1 for obj in objs if any(k[0] == family for k in obj)) == 1, family


def test_cases_are_what_the_inventory_says():
    """one forward case per compiled forward kernel (no covering sample), one reverse case per (W, NG, TSUM), the smallest shapes, the
    edges of the selection rules, and the cases that need a process of their own"""
    first = {}
    for c in TI._forward_cases():
        k, = [k for k in TI.reaches(c) if k[0] == 'fwd']
        assert k not in first, (k, TI.cid(c))
        first[k] = c
        dyn, points = k[3], c.N * c.L
        assert (points == 65 and c.max_blocks == 1) if dyn else (15 <= points <= 17 and c.max_blocks == 0), TI.cid(c)
    assert len(first) == 48
    for dyn in (False, True):                        # every ngrad kind with either schedule: 0, 1, 17 (a ragged second tile) and N
        kinds = {c.ngrad for k, c in first.items() if k[3] == dyn}
        assert kinds >= {0, 1, 17} and any(c.ngrad == c.N and c.N % 16 for k, c in first.items() if k[3] == dyn), kinds
    assert {(c.N, c.L) for k, c in first.items() if not k[3] and c.mode == 'path'} == {(5, 3), (17, 1)}
    for vks, ds in ((6, {24}), (13, {25, 53, 126}), (-1, {25, 53})):
        assert {c.d for k, c in first.items() if k[4] == vks and k[1] <= 64} == ds
    rec = collections.Counter(k for c in TI._record_cases() for k in TI.reaches(c) if k[0] == 'rec')
    assert len(rec) == 24 and {c.d for c in TI._record_cases()} >= {46, 47, 94, 95, 126}
    assert {c.q for c in TI._record_cases()} == {0, 1, 9, 16, 17}
    for c in TI._record_cases():
        k = TI.reaches(c)[-1]
        assert ((c.N, c.L) in ((64, 2), (128, 3))) if k[4] else (c.N == 17), TI.cid(c)
    assert {(c.d, c.N) for c in TI._recompute_cases()} == {(d, N) for d in (62, 63, 126) for N in (1, 17, 65)}
    assert {c.ngrad for c in TI.CASES} >= {0, 1, 17} and {c.N for c in TI.CASES if c.ngrad == c.N and c.N % 16} >= {5, 13, 17}
    assert {c.W for c in TI._generic_cases()} == {1, 17, 49, 51, 127} and {c.q for c in TI._generic_cases()} == {0, 1, 16}
    assert all(c.N * c.L == 17 for c in TI._generic_cases())
    assert sorted(c.W for c in TI._tiled_cases()) == [64, 65, 129, 193]
    behind = collections.Counter(tuple(sorted(TI.switches(c))) for c in TI.CASES if not TI.in_process(c))
    assert behind == {('XW_DISC_VIN_LDS',): 8, ('XW_DISC_DYNAMIC',): 4}
    # the rotated first round: more tiles than waves in the static kernel (rot = ntiles % G != 0)
    for c in TI.CASES:
        if not c.dynamic:
            assert c.max_blocks == 1 and (c.N * c.L + 15) // 16 == 5 and any(k[0] == 'fwd' and not k[3] for k in TI.reaches(c))
    # the rules at their edges
    at = lambda d, **kw: TI.reaches(TI.launch('bwd', 50, 9, d, 17, 1, **kw))             # noqa: E731
    assert [at(d, record=True)[0][4] for d in (24, 25, 52, 53)] == [6, 13, 13, 13]
    assert [at(d, record=True)[1][3] for d in (46, 47, 94, 95)] == [1, 2, 2, 3]
    assert [at(d)[0][3] for d in (62, 63)] == [1, 2]
    assert TI.reaches(TI.launch('bwd', 64, 9, 5, 17, 1)) == [('fwd', 64, True, False, 6), ('rec', 64, 0, 1, False)]
    assert TI.reaches(TI.launch('fwd', 96, 1, 5, 1025 * 16, 1, max_blocks=0)) == [('fwd', 96, False, False, 0)]
    assert TI.reaches(TI.launch('fwd', 96, 1, 5, 2049 * 16, 1, max_blocks=0)) == [('fwd', 96, False, True, 0)]


def test_parser_reads_the_profiler_spelling():
    """the first k_disc_fwd and k_disc_rec line of profiles/r06_rocprofv3_kernel_stats.csv, and the tuples back to cases that reach them"""
    stats = open(os.path.join(TI.ROOT, 'profiles', 'r06_rocprofv3_kernel_stats.csv')).read().splitlines()
    a = next(ln for ln in stats if 'k_disc_fwd<' in ln)
    b = next(ln for ln in stats if 'k_disc_rec<' in ln)
    assert TI.parse_kernel(a) == ('fwd', 50, False, True, 6) and TI.parse_kernel(b) == ('rec', 50, 0, 1, True)
    want = TI.reached()
    assert want[TI.parse_kernel(a)] and want[TI.parse_kernel(b)]
    ode = [ln for ln in stats if 'k_ode_' in ln]
    assert ode and all(TI.parse_kernel(ln) is None for ln in ode)
    assert TI.parse_kernel('(anonymous namespace)::k_disc_cot(double const*, double const*)') is None
    assert TI.parse_kernel('(anonymous namespace)::k_disc_xproj(double const*, double const*, int, int, int, double*)') == ('xproj',)
    assert TI.parse_kernel('void (anonymous namespace)::k_disc_fwd<128, false, false, -1>(double const*)') == ('fwd', 128, False, False, -1)
    assert TI.parse_kernel('void (anonymous namespace)::k_disc_bwd<50, 9, 2, false, true>(double const*)') == ('bwd', 50, 9, 2, False, True)
    assert TI.parse_kernel('void (anonymous namespace)::k_dt_bwd<12>(double const*)') == ('t_bwd', 12)
    assert TI.parse_kernel('(anonymous namespace)::kg_disc_fwd(double const*)') == ('g_fwd',)


# ---- the comparison helper cannot pass on a slightly wrong result ------------------------------------------------------------------
def _stand_in(c):
    """a CPU arena whose outputs hold the oracle's own results, as a device that computes exactly would leave them"""
    import test_gpu_testnet_inventory as T
    ref = T.reference(c)
    arena = G.Arena(torch.device('cpu'), chunk=1 << 18)
    ops = T.operands(arena, c, ref)
    P = c.N * c.L
    ops['v'].copy_(ref['v'].view(c.L, c.N))
    ops['vt'].copy_(ref['gX'][:, 0].reshape(c.L, c.N))
    ops['gxv'].copy_(ref['gX'][:c.ngrad, 1:].t())
    ops['gtv'].copy_(ref['gX'][:c.ngrad, 0])
    ops['act'].zero_()
    ops['gslab'].zero_()
    ops['gslab'][0].copy_(ref['gphi'])
    assert P > c.ngrad > 0
    return T, arena, ops, ref


def test_the_comparison_fails_on_a_slightly_wrong_result():
    c = TI.launch('bwd', 50, 9, 5, 17, 3, record=True, ngrad=17)
    T, arena, ops, ref = _stand_in(c)
    T.verify(arena, c, ops, ref)                     # the oracle's own results pass
    # one entry of the Vh.b gradient off by 1e-8 relative (the largest one: the metric is relative to the block's scale)
    W, d = c.W, c.d
    off = W * (d + 1) + W + W * W
    blk = ops['gslab'][0, off:off + W]
    assert torch.equal(blk, ref['gphi'][off:off + W]) and ref['phi']['Vh_b'].numel() == W
    i = int(blk.abs().argmax())
    keep = float(blk[i])
    blk[i] = keep * (1 + 1e-8)
    with pytest.raises(AssertionError, match='phi gradient Vh_b'):
        T.verify(arena, c, ops, ref)
    blk[i] = keep
    # one column of v swapped with its neighbour
    v = ops['v']
    keep = v.clone()
    v[:, 3], v[:, 4] = keep[:, 4], keep[:, 3]
    with pytest.raises(AssertionError, match='v: max rel'):
        T.verify(arena, c, ops, ref)
    v.copy_(keep)
    # one gxv entry left at the arena's pattern
    gx = ops['gxv']
    keep = float(gx[2, 16])
    gx.view(torch.int64)[2, 16] = G.PATTERN
    with pytest.raises(AssertionError, match=r'gxv#\d+: element \(2, 16\) was not written'):
        T.verify(arena, c, ops, ref)
    gx[2, 16] = keep
    # one guard double behind gxv overwritten
    chunk, first, _ = arena._where(gx)
    e = first + gx.numel()
    assert bool(chunk.guard[e]) and int(chunk.raw[e]) == G.PATTERN
    chunk.f64[e] = 0.0
    with pytest.raises(AssertionError, match=r'guard band overwritten.*1 doubles behind the end of gxv'):
        T.verify(arena, c, ops, ref)
    chunk.raw[e] = G.PATTERN
    T.verify(arena, c, ops, ref)                     # and everything put back passes again


def test_oracle_spread_table_still_holds():
    """the spreads stored in tests/test_gpu_testnet_inventory.ORACLE_SPREAD are what that file's tolerances rest on: measured again
    here (CPU), every spread is below an eighth of its tolerance -- or the widened tolerance is in force -- and within 16 x of the
    stored figure (rounding depends on the CPU's summation order; an orphaned table is off by far more or by a case)"""
    import test_gpu_testnet_inventory as T
    assert T.ORACLE_SPREAD
    for c in TI.CASES:
        if not T._corner(c):
            assert T._tolerances(c) == (T.TOL_VALUE, T.TOL_TANGENT, T.TOL_GRAD)
            continue
        stored, got = T.ORACLE_SPREAD[TI.cid(c)], T.oracle_spread(c)
        print(TI.cid(c), 'stored', stored, 'measured', got)
        for s_, g_, tol, used in zip(stored, got, (T.TOL_VALUE, T.TOL_TANGENT, T.TOL_GRAD), T._tolerances(c)):
            assert (s_ < tol / 8 and g_ < tol / 8 and used == tol) or (used == 8 * s_ and g_ < used / 4), (TI.cid(c), stored, got)
            assert g_ <= 16 * s_ and s_ <= 16 * max(g_, 1e-17), (TI.cid(c), stored, got)
