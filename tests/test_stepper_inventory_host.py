"""The fused stepper's inventory (tests/stepper_inventory.py) against the built library: every compiled stepper kernel is reached by a
form of a case of tests/test_gpu_stepper_inventory.py, and every form lands on a kernel that exists.  CPU only."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stepper_inventory as SI  # noqa: E402


def test_every_compiled_stepper_kernel_is_reached_and_every_form_lands_on_one():
    from xnode_wan_pde_solver_amd import _lib, kernels as KN
    assert tuple(KN.ODE_WIDTHS) == SI.ODE_WIDTHS and tuple(KN.METHODS) == SI.METHODS
    assert [KN.METHODS[n] for n in SI.METHODS] == [0, 1, 2]
    assert len(SI.CASES) == 90 and len(set(SI.CASES)) == 90
    have = SI.compiled(_lib.LIB_PATH)
    want = SI.reached()
    print('compiled stepper kernels: %d; reached: %d' % (len(have), len(want)))
    assert not have - set(want), 'compiled, but no case runs them: %s' % sorted(have - set(want), key=repr)
    assert not set(want) - have, 'forms that land on a kernel the library does not hold: %s' % sorted(
        (k, want[k]) for k in set(want) - have)
    # x_from_store and x_from_xstore share their kernel by design (two producers of one sweep); no other two forms of a case do
    for k, users in want.items():
        forms = sorted(f for _, f in users)
        assert len({c for c, _ in users}) == 1 and forms in ([forms[0]], ['x_from_store', 'x_from_xstore']), (k, users)
    # all instantiations of one kernel template at one width sit in one code object (what else a translation unit holds moves code
    # generation); the recomputing k_ode_bwd (SAVED false: the width's _recomp object) count as a group of their own
    objs = SI.code_objects(_lib.LIB_PATH)
    group = lambda k: (k[0], k[1], k[2]) + ((k[6],) if k[0] == 'bwd' else ())      # noqa: E731
    groups = {group(k) for k in have}
    assert len(groups) == 2 * 6 + 4                  # fwd, fwd_n4, bwd from the store, recomputing bwd, bwd_duo, bwd_n4; no narrow tiles at (64, 16)
    for g in sorted(groups, key=repr):
        assert sum(1 for obj in objs if any(group(k) == g for k in obj)) == 1, g
    # and what shares a code object, as csrc/xw_ode.hip says why: per width the forward kernels and the sweeps from the store in one,
    # the recomputing sweeps in another
    for obj in objs:
        assert len({(k[1], k[2]) for k in obj}) == 1 and len({k[0] == 'bwd' and not k[6] for k in obj}) == 1, sorted(obj, key=repr)[:3]
    assert len(objs) == 2 * len(SI.ODE_WIDTHS)


def test_forms_per_case():
    """what a case is made of: 15 forms in the 4x4x4 containers with a store, 10 at (64, 16), 6 / 5 for rk4"""
    n = {c: len(SI.forms_of(*c)) for c in SI.CASES}
    assert {(H, method): n[(H, K, 8, method)] for H, K in SI.ODE_WIDTHS for method in SI.METHODS} == {
        (20, 'euler'): 15, (20, 'midpoint'): 15, (20, 'rk4'): 6, (32, 'euler'): 15, (32, 'midpoint'): 15, (32, 'rk4'): 6,
        (64, 'euler'): 10, (64, 'midpoint'): 10, (64, 'rk4'): 5}
    assert all(n[(H, K, m, method)] == n[(H, K, 8, method)] for H, K, m, method in SI.CASES)


def test_parser_reads_the_profiler_spelling():
    """two lines of profiles/r02_rocprofv3_kernel_stats.csv, and the tuple back to the form that reaches it"""
    a = ('"void (anonymous namespace)::k_ode_bwd_duo<20, 10, 8, 1>((anonymous namespace)::BwdJobs, double const*, double const*, int, '
         'int)",348,60778864,174651.908046,27.68,110561,229002,16825.158625')
    b = ('"void (anonymous namespace)::k_ode_bwd<20, 10, 8, 1, false, true, false>((anonymous namespace)::BwdJobs, double const*, '
         'double const*, int, int)",87,8736060,100414.482759,3.98,72161,126160,17270.299863')
    stats = open(os.path.join(SI.ROOT, 'profiles', 'r02_rocprofv3_kernel_stats.csv')).read().splitlines()
    assert a in stats and b in stats
    assert SI.parse_kernel(a) == ('bwd_duo', 20, 10, 8, 1) == SI.reaches(20, 10, 8, 'midpoint', 'duo')
    assert SI.parse_kernel(b) == ('bwd', 20, 10, 8, 1, False, True, False) == SI.reaches(20, 10, 8, 'midpoint', 'x_from_store')
    assert SI.reaches(20, 10, 8, 'midpoint', 'x_from_xstore') == SI.parse_kernel(b)
    assert SI.parse_kernel('"void (anonymous namespace)::n4::k_ode_fwd_n4<32, 12, 3, 0, 2>((anonymous namespace)::FwdJobs, double '
                           'const*, double const*, int, int)",1,2,3') == ('fwd_n4', 32, 12, 3, 0, 2)
    assert SI.parse_kernel('"void (anonymous namespace)::k_tiled_fwd<1, 0>(int)",1,2,3') is None


def test_oracle_spread_table_still_holds():
    """the spreads stored in tests/test_gpu_stepper_inventory.ORACLE_SPREAD are what that file's tolerances rest on: measured again
    here (CPU, a second per case), every spread is below an eighth of its tolerance -- the project's tolerances stand -- and within
    16 x of the stored figure (rounding depends on the CPU's summation order; an orphaned table is off by far more or by a case)"""
    import test_gpu_stepper_inventory as T
    for c, stored in T.ORACLE_SPREAD.items():
        got = T.oracle_spreads(c)
        print(T._cid(c), 'stored', stored, 'measured', got)
        for s_, g_, tol in zip(stored, got, (T.TOL_VALUE, T.TOL_GRAD, T.TOL_GRAD)):
            assert s_ < tol / 8 and g_ < tol / 8, (c, stored, got)
            assert g_ <= 16 * s_ and s_ <= 16 * max(g_, 1e-17), (c, stored, got)
        assert T._tolerances(c) == (T.TOL_VALUE, T.TOL_GRAD, T.TOL_GRAD)
