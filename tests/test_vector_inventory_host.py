"""The vector-ALU steppers' inventory (tests/vector_inventory.py) against the built library and against its own claims: the coverage
tables hold, every dopri5 fixture is what the table says on the restatement alone, every compiled kd_* / kg_ode_* kernel is reached by
a case of tests/test_gpu_vector_paths.py and every case lands on kernels that exist; that file's spread table still holds.  CPU only."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vector_inventory as VI  # noqa: E402


def test_generic_coverage():
    """every value of every axis with every method and with every sweep mode; every N at the widest and at the narrowest width;
    the deepest field with rk4; two-job calls pair N across a block / slab edge"""
    C = VI.GENERIC_CASES
    assert not VI.missing(C, VI.GENERIC_AXES, VI.GENERIC_PARTNERS)
    assert VI.GENERIC_AXES['N'] == (1, 15, 16, 17, 63, 64, 65) and VI.GENERIC_AXES['m'] == (1, 2, 10, 11, 32)
    assert set(VI.GENERIC_AXES['HK']) == {(1, 1), (5, 3), (24, 13), (33, 9), (63, 15), (64, 16), (20, 10)}
    assert VI.GENERIC_AXES['d'] == (1, 5, 17, 126) and VI.GENERIC_AXES['L'] == (1, 2, 3)
    for HK in ((64, 16), (1, 1)):
        assert {c['N'] for c in C if c['HK'] == HK} == set(VI.NS), HK
    assert any(c['m'] == 32 and c['method'] == 'rk4' for c in C)
    assert all(c['m'] >= 11 for c in C if c['HK'] in VI.DEEP_ONLY) and {c['m'] for c in C if c['HK'] in VI.DEEP_ONLY} == {11, 32}
    assert all(VI.SECOND_N[n] != n and VI.SECOND_N[n] in VI.NS for n in VI.NS)
    assert 30 <= len(C) <= 60, len(C)
    from xnode_wan_pde_solver_amd import kernels as KN
    for c in C:                                             # widths the C ABI hands to xw_generic.hip as they are
        assert KN.ode_generic(c['H'], c['K'], c['m']), VI.gid(c)
        if c['m'] > 10:                                     # ... and, above depth 10, the shapes the engine itself sends there
            assert KN.stepper_family(c['H'], c['K'], c['m']) == 'generic' and KN.ode_container(c['H'], c['K'], c['m']) == (c['H'], c['K'])


def test_dopri5_coverage():
    """every value of every axis with both instantiations, every sweep mode with every cotangent form; the <64> layouts; the job
    counts; growth, the duplicate time and a rejecting fixture with either instantiation"""
    C = VI.DOPRI_COVER
    assert not VI.missing(C, VI.DOPRI_AXES, VI.DOPRI_PARTNERS, VI.DOPRI_PAIRS)
    assert VI.DOPRI_AXES['L'] == (2, 3, 5) and VI.DOPRI_AXES['jobs'] == (1, 2, 8) and VI.JOBS_2 == (17, 65) and len(VI.JOBS_8) == 8
    inst = lambda c: VI.reaches_dopri(c)[0][1]                                  # noqa: E731
    for c in C:
        assert inst(c) == c['inst'] and (c['H'], c['K'], c['m']) in VI.NETS[c['inst']], VI.did(c)
    for hm in (32, 64):
        assert {(c['H'], c['K'], c['m']) for c in C if c['inst'] == hm} == set(VI.NETS[hm]), hm
        assert {(c['H'], c['K'], c['m']) for c in C if c['inst'] == hm and VI.integrates(c)} == set(VI.NETS[hm]), hm
    assert set(VI.LAYOUTS_64.values()) <= set(VI.NETS[64])
    assert any(not VI.integrates(c) for c in C)             # (and one that does not: the forward ends in kd_init2)
    assert VI.container(33, 9, 8) == VI.container(48, 16, 10) == (64, 16) and VI.container(33, 9, 11) == (33, 9)
    assert VI.container(64, 16, 32) == (64, 16) and VI.container(20, 13, 2) == (64, 16)       # (K alone forces the wide container)
    assert VI.container(24, 13, 11) == (24, 13) and VI.container(12, 6, 8) == (20, 10) and VI.container(24, 11, 10) == (32, 12)
    both = VI.DOPRI_COVER + VI.DOPRI_EXACT
    for hm in (32, 64):
        mine = [c for c in both if inst(c) == hm]
        assert {c['N'] for c in mine if c['jobs'] == 1} == set(VI.NS), hm
        assert {True, False} == {c['grow'] for c in mine} == {c['dup'] for c in mine}
        assert any(c['exact'] and (c['seed'], c['scale']) in VI.REJECTING for c in mine), hm
        assert any(c['exact'] and c['dup'] and c['L'] >= 3 for c in mine) and any(c['exact'] and c['N'] == 1 for c in mine)
    assert [VI.instantiation(h) for h in (1, 32, 33, 64)] == [32, 32, 64, 64]


def test_exact_fixtures_on_the_restatement():
    """every exact-decision fixture: tanh-only, gap > 1e-9, the attempts and accepted steps the table states; the rejection fixtures
    reject; the duplicate-time fixtures read y0 at t[1] and keep the gap of the plain fixture"""
    import test_gpu_vector_paths as T
    from test_gpu_dopri5 import _ref_Y
    gaps = {}
    for c in VI.DOPRI_EXACT:
        assert c['m'] == 1 and c['jobs'] == 1
        cfg, theta, t, ((X, s),) = T._dopri_samples(c)
        ys, info = _ref_Y(theta, cfg, X, s)
        print(VI.did(c), 'gap %.3g' % info['gap'], (info['n_att'], info['n_acc']))
        assert info['gap'] > 1e-9, VI.did(c)
        assert c['counts'] is None or c['counts'] == (info['n_att'], info['n_acc']), VI.did(c)
        rejecting = (c['seed'], c['scale']) in VI.REJECTING
        assert (info['n_att'] > info['n_acc']) == rejecting, VI.did(c)
        if c['dup']:
            assert float(t[1]) == float(t[0]) and torch.equal(ys[:, 1], ys[:, 0]) and info['steps'][0][0] == float(t[0])
        gaps.setdefault((c['seed'], c['scale']), {})[c['dup']] = info['gap']
    twins = [g for g in gaps.values() if len(g) == 2]
    assert twins and all(g[True] == g[False] for g in twins)
    assert len({(s_, x_) for s_, x_ in VI.REJECTING}) == len(VI.REJECTING) and all(k in gaps for k in VI.REJECTING)


def test_every_compiled_vector_kernel_is_reached_and_every_case_lands_on_one():
    from xnode_wan_pde_solver_amd import _lib
    have = VI.compiled(_lib.LIB_PATH)
    want = VI.reached()
    print('compiled kd_* / kg_ode_* kernels: %d; reached: %d' % (len(have), len(want)))
    assert not have - set(want), 'compiled, but no case runs them: %s' % sorted(have - set(want), key=repr)
    assert not set(want) - have, 'cases that land on a kernel the library does not hold: %s' % sorted(
        ((k, want[k][:3]) for k in set(want) - have), key=repr)
    # what the library holds today (a change detector beside the set equality)
    assert have == {(k, hm) for k in VI.DOPRI_KERNELS for hm in (32, 64)} | {(k,) for k in VI.GENERIC_KERNELS}
    # every instantiation is reached by covering cases AND by exact-decision fixtures, the generic pair by the tail cases too
    for k in have:
        kinds = {i.split('-')[0] for i in want[k]}
        assert kinds >= ({'cover', 'exact'} if k[0] in VI.DOPRI_KERNELS else {'tail'}), (k, kinds)


def test_parser_reads_both_spellings():
    assert VI.parse_kernel('void (anonymous namespace)::kd_sweep<64>((anonymous namespace)::Jobs<XwDopriSweepJob>, double const*)') == ('kd_sweep', 64)
    assert VI.parse_kernel('"void (anonymous namespace)::kd_init1<32>(Jobs<XwDopriJob>, double const*)",1,2,3') == ('kd_init1', 32)
    assert VI.parse_kernel('(anonymous namespace)::kg_ode_bwd(XwOdeBwdJob, double const*, double const*, int)') == ('kg_ode_bwd',)
    assert VI.parse_kernel('(anonymous namespace)::kg_disc_fwd(double const*)') is None
    assert VI.parse_kernel('void (anonymous namespace)::ktd_sweep<4>(int)') is None
    assert VI.parse_kernel('void (anonymous namespace)::k_ode_fwd<20, 10, 8, 1, 2>(int)') is None


def test_cotangent_forms_are_what_the_sweeps_form():
    """_cot_host against the definitions in csrc/xw_common.h, written out per element; in x_cot_ones form every cotangent is 1 at every
    time index >= 1 (to rounding, exactly for the stored and the residual forms) and keeps a value of its own at l = 0"""
    import test_gpu_vector_paths as T
    N, L = 5, 3
    u = torch.randn(L, N, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    for form in VI.COTS:
        for seed in (6, 7, 8, 9):                           # (seed mod 2: w per point; seed mod 3 == 0: c, c' tables)
            for ones in (False, True):
                f, cot = T._cot_host(form, ones, N, L, seed, u)
                assert cot.shape == (N, L)
                for n in range(N):
                    for l in range(L):
                        if form == 'ubar':
                            want = float(f['ubar'][l, n])
                        elif form == 'res':
                            want = f['res']['base'] + f['res']['coef'] * float(u[l, n] - f['res']['ref'][l, n])
                        elif form == 'res_first':
                            want = f['res']['base'] + (f['res']['coef'] * float(u[0, n] - f['res']['ref'][n]) if l == 0 else 0.0)
                        else:
                            r, wk = f['res'], f['res']['weak']
                            w = float(wk['w'][l, n] if wk['w'].dim() == 2 else wk['w'][n])
                            dcu = float(wk['c'][l, n] + u[l, n] * wk['cp'][l, n]) if 'c' in wk else 2 * wk['ckappa'] * float(u[l, n])
                            want = r['coef'] * dcu * float(r['ref'][l, n]) * w + (r['base'] * float(r['ref'][l, n]) if l == L - 1 else 0.0)
                        assert abs(float(cot[n, l]) - want) <= 1e-14 * max(1.0, abs(want)), (form, seed, ones, n, l)
                if ones:
                    assert float((cot[:, 1:] - 1.0).abs().max()) <= (0.0 if form != 'weak' else 4 * 2.0 ** -52), (form, seed)
                    assert float((cot[:, 0] - 1.0).abs().min()) > 1e-3
        assert {T._cot_host('weak', False, N, L, s_, u)[0]['res']['weak']['w'].dim() for s_ in (6, 7)} == {1, 2}
        assert 'c' in T._cot_host('weak', False, N, L, 6, u)[0]['res']['weak'] and 'ckappa' in T._cot_host('weak', False, N, L, 7, u)[0]['res']['weak']


def test_oracle_spread_table_still_holds():
    """the spreads stored in tests/test_gpu_vector_paths.ORACLE_SPREAD are what that file's tolerances rest on: measured again here
    (CPU), every spread is below an eighth of its tolerance -- the project's tolerances stand -- and within 16 x of the stored figure
    (rounding depends on the CPU's summation order; an orphaned table is off by far more or by a case)"""
    import test_gpu_vector_paths as T
    assert T.ORACLE_SPREAD
    for c in VI.GENERIC_CASES:
        if not T._corner(c):
            assert T._tolerances(c) == (T.TOL_VALUE, T.TOL_GRAD)
            continue
        stored, got = T.ORACLE_SPREAD[VI.gid(c)], T.oracle_spread(c)
        print(VI.gid(c), 'stored', stored, 'measured', got)
        for s_, g_, tol, used in zip(stored, got, (T.TOL_VALUE, T.TOL_GRAD), T._tolerances(c)):
            assert (s_ < tol / 8 and g_ < tol / 8 and used == tol) or (used == 8 * s_ and g_ < used / 4), (VI.gid(c), stored, got)
            assert g_ <= 16 * max(s_, 1e-17) and s_ <= 16 * max(g_, 1e-17), (VI.gid(c), stored, got)
