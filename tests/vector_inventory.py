"""The two stepper families on the vector ALU, their compiled kernels and the cases that reach them -- TEST INFRASTRUCTURE ONLY
(imported like tests/testnet_inventory.py, whose loader of tools/isa_same.py it shares through tests/stepper_inventory.py).  CPU only.

    the generic stepper    csrc/xw_generic.hip: kg_ode_fwd, kg_ode_bwd -- one lane per path, 64 lanes per block, one gradient slab per
                           16 paths; behind kernels.ode_fwd_multi / ode_bwd_multi at every width that is no MFMA container and at
                           every depth above 10 (kernels.ode_generic)
    the vector dopri5      csrc/xw_dopri.hip: kd_init1, kd_init2, kd_attempt, kd_sweep, each compiled twice (<32> for H <= 32, <64>
                           for 33 .. 64: instantiation() below restates that rule, once); behind kernels.dopri5_fwd / dopri5_sweep
                           with stepper='vector', at the widths kernels.ode_container gives a network (the container it is embedded
                           in, or its own widths above depth 10)

Two views of the kernel set, as in the other inventories: compiled(path) -- the kernel symbols of a built libxnwan.so, names only --
and reached() -- what the case tables below land on.  tests/test_vector_inventory_host.py asserts that the two are the same set and
that the tables cover what they say; tests/test_gpu_vector_paths.py runs every case against the oracle inside a guarded arena.

The tables are seeded covering selections (test_gpu_edges.cover), not products.

Generic stepper (GENERIC_CASES): every value of every axis with every method and with every sweep mode; every N with the (64, 16)
and with the (1, 1) width; u_layers = 32 with rk4.  Axes: the width (H, K), u_layers m, the path count N (the launch geometry's
edges: 64 lanes per block, 16 paths per slab), the number of sample times L, the dimension d, the cotangent form, the forward job
with / without Y, one job or two jobs of different N in one call.

Vector dopri5 (DOPRI_COVER + DOPRI_EXACT): every value of every axis with both instantiations, every sweep mode with every cotangent
form.  DOPRI_COVER is compared on the device's own accepted grid (ReLU fields: tests/test_gpu_dopri5.py says why); DOPRI_EXACT are
tanh-only fields (u_layers = 1) whose step decisions are pinned exactly: each has gap > 1e-9 on the restatement alone (asserted on
the CPU), the rejection fixtures take more attempts than they accept, the duplicate-time fixtures have t[1] == t[0].
"""
import os
import random
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stepper_inventory import ROOT, isa_same  # noqa: E402,F401
if __name__ == '__main__':
    sys.path.insert(0, ROOT)
from test_gpu_edges import D_MAX, cover, missing  # noqa: E402

_NAME = re.compile(r'(?<![\w])(kd_init1|kd_init2|kd_attempt|kd_sweep|kg_ode_fwd|kg_ode_bwd)(?:<([^<>]*)>)?\(')
DOPRI_KERNELS = ('kd_init1', 'kd_init2', 'kd_attempt', 'kd_sweep')
GENERIC_KERNELS = ('kg_ode_fwd', 'kg_ode_bwd')


def parse_kernel(text):
    """('kd_sweep', 64) / ('kg_ode_bwd',) of a demangled name as llvm-objdump and rocprofv3 spell it; None if `text` names none of
    the two families' kernels"""
    m = _NAME.search(text)
    if m is None:
        return None
    args = () if m.group(2) is None else tuple(int(a) for a in m.group(2).split(','))
    assert len(args) == (1 if m.group(1) in DOPRI_KERNELS else 0), text
    return (m.group(1),) + args


def compiled(path):
    """the set of kd_* / kg_ode_* kernel tuples in `path` (a libxnwan.so or one object).  Reads the function symbols of .text
    (llvm-objdump -t --demangle) of every gfx950 code object; never an instruction."""
    found = set()
    with tempfile.TemporaryDirectory() as tmp:
        for co in isa_same.bundles(path, tmp):
            for line in isa_same.run(isa_same.LLVM + '/llvm-objdump', '-t', '--demangle', co).splitlines():
                if re.match(r'^[0-9a-f]+ \S+\s+F \.text\s', line):
                    k = parse_kernel(line)
                    if k is not None:
                        assert k not in found, 'compiled twice: %r' % (k,)
                        found.add(k)
    return found


def instantiation(Hc):
    """xw_dopri5_init / _attempts / _sweep: the <HM> a launch at blob width Hc lands on"""
    return 32 if Hc <= 32 else 64


# ---- the generic stepper -----------------------------------------------------------------------------------------------------------
METHODS = ('euler', 'midpoint', 'rk4')
MODES = ('x', 'params', 'both', 'both_ones')                # want_x / want_params / both / both with x_cot_ones
COTS = ('ubar', 'res', 'res_first', 'weak')
NS = (1, 15, 16, 17, 63, 64, 65)
DEEP_ONLY = ((20, 10), (64, 16))                            # MFMA containers: on the generic path above depth 10 only (the engine's shapes)
GENERIC_AXES = {
    'HK': ((1, 1), (5, 3), (24, 13), (33, 9), (63, 15)) + DEEP_ONLY,
    'm': (1, 2, 10, 11, 32),
    'N': NS,
    'L': (1, 2, 3),
    'd': (1, 5, 17, D_MAX),
    'cot': COTS,
    'Y': (True, False),                                     # the forward job with / without Y (the sweep's checkpoints need one with)
    'jobs': (1, 2),
}
GENERIC_PARTNERS = {'method': METHODS, 'mode': MODES}
SECOND_N = {1: 17, 15: 64, 16: 65, 17: 1, 63: 16, 64: 15, 65: 63}      # the other job of a two-job call: across a block / slab edge


def _deep(rnd, c):
    if c['HK'] in DEEP_ONLY and c['m'] <= 10:
        c['m'] = rnd.choice((11, 32))


def _generic_cases():
    cases = cover(GENERIC_AXES, GENERIC_PARTNERS, fixed=_deep, seed=29)
    rnd = random.Random(31)
    for HK in ((64, 16), (1, 1)):                           # every N with the widest and with the narrowest width
        for N in NS:
            if not any(c['HK'] == HK and c['N'] == N for c in cases):
                c = {k: rnd.choice(list(v)) for k, v in list(GENERIC_AXES.items()) + list(GENERIC_PARTNERS.items())}
                c.update(HK=HK, N=N)
                _deep(rnd, c)
                cases.append(c)
    for i, c in enumerate(cases):
        c['H'], c['K'] = c['HK']
        c['seed'] = 1100 + i
    return cases


def gid(c):
    return '%s-%s-%s-N%d%s-H%dK%dm%d-d%d-L%d%s' % (c['method'], c['mode'], c['cot'], c['N'], '+%d' % SECOND_N[c['N']] if c['jobs'] == 2 else '',
                                                   c['H'], c['K'], c['m'], c['d'], c['L'], '' if c['Y'] else '-noY')


GENERIC_CASES = _generic_cases()
assert not missing(GENERIC_CASES, GENERIC_AXES, GENERIC_PARTNERS), missing(GENERIC_CASES, GENERIC_AXES, GENERIC_PARTNERS)
assert len({gid(c) for c in GENERIC_CASES}) == len(GENERIC_CASES)


def generic_Ns(c):
    return (c['N'], SECOND_N[c['N']]) if c['jobs'] == 2 else (c['N'],)


# ---- the vector dopri5 -------------------------------------------------------------------------------------------------------------
# networks (u_hidden_dim, u_hidden_hidden_dim, u_layers) per instantiation, by layout: embedded in a container (Hn < H or K below the
# container's), a container's own widths, the network's own widths above depth 10
NETS = {
    32: ((12, 6, 8), (20, 10, 1), (24, 11, 10), (32, 12, 2), (24, 13, 11), (1, 1, 11), (32, 16, 32)),
    64: ((33, 9, 8), (48, 16, 10), (20, 13, 2), (33, 9, 11), (64, 16, 32), (64, 16, 1)),
}
LAYOUTS_64 = {'embedded Hn=33': (33, 9, 8), 'embedded Hn=48': (48, 16, 10), 'own widths m=11 H=33': (33, 9, 11), '(64, 16) m=32': (64, 16, 32)}
DOPRI_AXES = {
    'net': tuple(range(max(len(v) for v in NETS.values()))),                # index into NETS[inst] (modulo its length)
    'N': NS,
    'd': (1, 5, 17, D_MAX),
    'L': (2, 3, 5),
    'mode': MODES,
    'cot': COTS,
    'jobs': (1, 2, 8),
    'grow': (False, True),                                  # cap=2, chunk=3: the record grows on the host between chunks
    'dup': (False, True),                                   # t[1] == t[0]
}
DOPRI_PARTNERS = {'inst': (32, 64)}
DOPRI_PAIRS = (('mode', 'cot'),)
JOBS_2, JOBS_8 = (17, 65), (1, 15, 16, 17, 63, 64, 65, 33)


def _dopri_fixed(rnd, c):
    if c['jobs'] == 2:
        c['N'] = JOBS_2[0]
    elif c['jobs'] == 8:
        c['N'] = JOBS_8[0]


def integrates(c):
    """False where the sample times do not lie past t[0] (two times, the second equal to the first): the controller starts done"""
    return not (c['dup'] and c['L'] == 2)


def _dopri_cover():
    cases = cover(DOPRI_AXES, DOPRI_PARTNERS, DOPRI_PAIRS, fixed=_dopri_fixed, seed=37)
    rnd = random.Random(41)
    for inst, nets in NETS.items():                         # every network with a case that integrates (t[L - 1] past t[0]: attempts run)
        for i in range(len(nets)):
            if not any(c['inst'] == inst and c['net'] % len(nets) == i and integrates(c) for c in cases):
                c = {k: rnd.choice(list(v)) for k, v in list(DOPRI_AXES.items()) + list(DOPRI_PARTNERS.items())}
                c.update(inst=inst, net=i, dup=False)
                _dopri_fixed(rnd, c)
                cases.append(c)
    for i, c in enumerate(cases):
        nets = NETS[c['inst']]
        c['H'], c['K'], c['m'] = nets[c['net'] % len(nets)]
        c.update(seed=1300 + i, scale=1.0, exact=False)
    return cases


def dopri_Ns(c):
    return JOBS_2 if c['jobs'] == 2 else JOBS_8 if c['jobs'] == 8 else (c['N'],)


# tanh-only fixtures of tests/test_gpu_dopri5._case: (d, H, K, N, L, seed), start multiplier, t[1] == t[0], (attempts, accepted) of the
# restatement, sweep mode, cotangent form, grows.  Every one has gap > 1e-9 on the restatement (the host test measures it again).
_EXACT = (
    # <64>
    ((3, 33, 9, 1, 3, 201), 1.0, False, (7, 7), 'both', 'ubar', False),
    ((5, 48, 16, 17, 4, 202), 1.0, False, (7, 7), 'x', 'res', False),
    ((20, 64, 16, 65, 5, 203), 1.0, True, (7, 7), 'params', 'weak', False),
    ((4, 64, 13, 16, 2, 204), 1.0, False, (6, 6), 'both_ones', 'res_first', False),
    ((D_MAX, 40, 16, 15, 3, 205), 1.0, False, (6, 6), 'both', 'weak', True),
    ((2, 33, 13, 64, 4, 206), 1.0, False, (8, 8), 'params', 'res_first', False),
    ((3, 33, 9, 1, 3, 201), 30.0, False, (8, 5), 'x', 'weak', False),
    ((2, 33, 13, 64, 4, 206), 300.0, False, (6, 5), 'both_ones', 'ubar', True),
    ((3, 33, 9, 1, 3, 201), 1.0, True, (7, 7), 'params', 'ubar', False),
    # <32>
    ((3, 12, 6, 1, 3, 211), 1.0, False, (6, 6), 'both', 'res', False),
    ((5, 20, 10, 17, 4, 212), 1.0, False, (8, 8), 'x', 'ubar', True),
    ((20, 32, 12, 65, 5, 213), 1.0, True, (7, 7), 'params', 'res', False),
    ((4, 24, 11, 16, 2, 214), 1.0, False, (7, 7), 'both_ones', 'weak', False),
    ((D_MAX, 32, 12, 15, 3, 215), 1.0, False, (5, 5), 'both', 'res_first', False),
    ((2, 1, 1, 64, 4, 216), 1.0, False, (5, 5), 'x', 'res_first', False),
    ((3, 12, 6, 1, 3, 211), 30.0, False, (4, 4), 'both_ones', 'res', False),
    ((2, 20, 10, 63, 4, 217), 1.0, False, (9, 9), 'params', 'weak', False),
    ((5, 20, 10, 17, 4, 212), 100.0, False, (8, 7), 'both', 'weak', False),
)
REJECTING = ((201, 30.0), (206, 300.0), (212, 100.0))         # (seed, start multiplier): n_att > n_acc on the restatement


def _dopri_exact():
    out = []
    for (d, H, K, N, L, seed), scale, dup, counts, mode, cot, grow in _EXACT:
        out.append(dict(d=d, H=H, K=K, m=1, N=N, L=L, seed=seed, scale=scale, dup=dup, counts=counts, mode=mode, cot=cot, grow=grow,
                        jobs=1, exact=True, inst=None))
    return out


def did(c):
    return '%s-%s-%s-N%s-H%dK%dm%d-d%d-L%d-s%d%s%s%s' % (
        'exact' if c['exact'] else 'cover', c['mode'], c['cot'], '+'.join(str(n) for n in dopri_Ns(c)), c['H'], c['K'], c['m'], c['d'],
        c['L'], c['seed'], '-x%g' % c['scale'] if c['scale'] != 1.0 else '', '-grow' if c['grow'] else '', '-dup' if c['dup'] else '')


DOPRI_COVER = _dopri_cover()
DOPRI_EXACT = _dopri_exact()
assert not missing(DOPRI_COVER, DOPRI_AXES, DOPRI_PARTNERS, DOPRI_PAIRS)
assert len({did(c) for c in DOPRI_COVER + DOPRI_EXACT}) == len(DOPRI_COVER) + len(DOPRI_EXACT)
# the tail that exists twice (kg_ode_bwd's and kd_sweep's copy of the l = 0 read-out and lift): L = 1, widths both families run at
# their own -- (H, K, m, N, d); every sweep mode and cotangent form at each
TAIL_CASES = ((33, 9, 11, 17, 5), (64, 16, 32, 65, 17), (1, 1, 11, 1, 1), (24, 13, 12, 16, D_MAX))


def container(H, K, m):
    """kernels.ode_container (asked of the library: the widths a network's blob is laid out at)"""
    from xnode_wan_pde_solver_amd import kernels as KN
    return KN.ode_container(H, K, m)


def reaches_generic(c):
    return [(k,) for k in GENERIC_KERNELS]


def reaches_dopri(c):
    hm = instantiation(container(c['H'], c['K'], c['m'])[0])
    return [(k, hm) for k in DOPRI_KERNELS]


def reached():
    """{kernel tuple: [case id, ...]} over every table"""
    out = {}
    for c in GENERIC_CASES:
        for k in reaches_generic(c):
            out.setdefault(k, []).append(gid(c))
    for c in DOPRI_COVER + DOPRI_EXACT:
        for k in reaches_dopri(c):
            out.setdefault(k, []).append(did(c))
    for H, K, m, N, d in TAIL_CASES:
        for k in reaches_generic(None) + reaches_dopri(dict(H=H, K=K, m=m)):
            out.setdefault(k, []).append('tail-H%dK%dm%d' % (H, K, m))
    return out


if __name__ == '__main__':
    print('generic stepper: %d cases; vector dopri5: %d covering + %d exact; tail: %d' % (
        len(GENERIC_CASES), len(DOPRI_COVER), len(DOPRI_EXACT), len(TAIL_CASES)))
    for c_ in GENERIC_CASES:
        print('| %s |' % gid(c_))
    for c_ in DOPRI_COVER + DOPRI_EXACT:
        print('| %s | <%d> |' % (did(c_), reaches_dopri(c_)[0][1]))
