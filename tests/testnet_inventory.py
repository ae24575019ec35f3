"""The test network's compiled kernels, and the launches that reach them -- TEST INFRASTRUCTURE ONLY (imported like
tests/stepper_inventory.py, whose loader of tools/isa_same.py it reuses).  CPU only.

csrc/xw_disc_fwd.hip, xw_disc_rec.hip and xw_disc_bwd.hip compile into one kernel per container width, record, schedule and input-layer
plan (k_disc_fwd), per width, input groups and path-group form (k_disc_rec), per cotangent groups and output (k_disc_bwd), and
k_disc_xproj -- all instantiations of one template in one code object (code_objects) --; csrc/xw_disc_tiled.hip into
one forward and one reverse kernel per row-tile count; csrc/xw_generic.hip holds the generic pair.  Two views of that set:

    compiled(path)   what a built libxnwan.so holds: the kernel symbols of its gfx950 code objects, names only (parse_kernel)
    reaches(launch)  what a case lands on, in launch order: a restatement of the dispatch in xw_disc_fwd_xproj, xw_disc_bwd,
                     xw_disc_gradx, XWD_DISPATCH (xw_disc_tiled.hip), the generic fall-through of the widths that are no container,
                     and of what kernels.disc_bwd / kernels.disc_gradx do where no recomputing kernel exists

tests/test_testnet_inventory_host.py asserts that the two are the same set; tests/test_gpu_testnet_inventory.py runs every case of
CASES against the oracle inside a guarded arena.

Kernel tuples:   ('fwd', W, ACT, DYN, VKS)           k_disc_fwd    ACT: stores the record; DYN: ticket queue; VKS: input-layer k-steps in
                                                                   LDS (0 none, 6, 13; -1: the x-projection table is handed in)
                 ('rec', W, Q, NG, TSUM)             k_disc_rec    Q = 0: rolled layer loop; NG: groups of 48 input rows; TSUM: the
                                                                   input layer's gradient once per path group
                 ('bwd', W, Q, CTG, PARAMS, INGRAD)  k_disc_bwd    the recomputing reverse (W = 50, Q = 9); CTG: groups of 64 input rows
                 ('xproj',)                          k_disc_xproj
                 ('t_fwd', NT), ('t_bwd', NT)        k_dt_fwd / k_dt_bwd, NT row tiles of 16
                 ('g_fwd',), ('g_bwd',)              kg_disc_fwd / kg_disc_bwd

A case (Launch) is what a caller of kernels.disc_xproj / disc_fwd / disc_bwd / disc_gradx passes:
    entry       'fwd'    disc_fwd (after disc_xproj when xproj=True)
                'bwd'    record=True: disc_fwd storing the record, then disc_bwd from it; record=False: disc_bwd alone (the recomputing
                         kernel at W = 50, q = 9; elsewhere the wrapper stores a record first: a forward plus a reverse)
                'gradx'  disc_gradx (the recomputing kernel at W = 50, q = 9; elsewhere the forward's fused gradient)
    family      'mfma' (the C entry points xw_disc_*: containers and, at any other width, the generic path) or 'tiled'
    W, q, d, N, L, mode ('path' | 'point': L = 1, a time per point), record, xproj (a table is passed; path mode), max_blocks
    (0: the default cap), ngrad, want_vt, and the three library switches disc_vin_lds, disc_dynamic, disc_rec_tsum (SWITCHES) as
    booleans (True: the default)
"""
import collections
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stepper_inventory import ROOT, isa_same  # noqa: E402,F401

CONTAINERS = (50, 64, 96, 128)                               # kernels.DISC_WIDTHS (asserted by the host test)
QMAX = 16                                                    # XW_QMAX: deepest network with the fused input gradient (MFMA, generic)
# a case's attribute -> the field of options.EngineOptions (kernels.switched takes it), and the field's variable for ids and messages
SWITCHES = {'vin_lds': 'disc_vin_lds', 'dynamic': 'disc_dynamic', 'rec_tsum': 'disc_rec_tsum'}
ENV = {field: 'XW_' + field.upper() for field in SWITCHES.values()}

_NAME = re.compile(r'(?<![\w])(k_disc_fwd|k_disc_rec|k_disc_bwd|k_disc_xproj|k_dt_fwd|k_dt_bwd|kg_disc_fwd|kg_disc_bwd)(?:<([^<>]*)>)?\(')
_FAMILY = {'k_disc_fwd': ('fwd', 4), 'k_disc_rec': ('rec', 4), 'k_disc_bwd': ('bwd', 5), 'k_disc_xproj': ('xproj', 0),
           'k_dt_fwd': ('t_fwd', 1), 'k_dt_bwd': ('t_bwd', 1), 'kg_disc_fwd': ('g_fwd', 0), 'kg_disc_bwd': ('g_bwd', 0)}


def parse_kernel(text):
    """the kernel tuple of a demangled name as llvm-objdump and rocprofv3 spell it ('void (anonymous namespace)::k_disc_fwd<50, true,
    true, 6>(double const*, ...)'); None if `text` names no test-network kernel (the stepper's, k_disc_cot, ...)"""
    m = _NAME.search(text)
    if m is None:
        return None
    family, nargs = _FAMILY[m.group(1)]
    args = () if m.group(2) is None else tuple(
        {'true': True, 'false': False}[a] if a in ('true', 'false') else int(a) for a in (s.strip() for s in m.group(2).split(',')))
    assert len(args) == nargs, text
    return (family,) + args


def code_objects(path):
    """the test-network kernel tuples of `path` (a libxnwan.so or one object), one set per gfx950 code object that holds any.  Reads the
    function symbols of .text (llvm-objdump -t --demangle); never an instruction."""
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for co in isa_same.bundles(path, tmp):
            found = set()
            for line in isa_same.run(isa_same.LLVM + '/llvm-objdump', '-t', '--demangle', co).splitlines():
                if re.match(r'^[0-9a-f]+ \S+\s+F \.text\s', line):
                    k = parse_kernel(line)
                    if k is not None:
                        assert k not in found, 'compiled twice: %r' % (k,)
                        found.add(k)
            if found:
                out.append(found)
    return out


def compiled(path):
    """the set of test-network kernel tuples in `path`, over all its code objects"""
    found = set()
    for obj in code_objects(path):
        assert not found & obj, 'compiled twice: %r' % sorted(found & obj, key=repr)
        found |= obj
    return found


# ---- a launch, as its caller describes it -------------------------------------------------------------------------------------------
Launch = collections.namedtuple('Launch', 'entry family W q d N L mode record xproj max_blocks ngrad want_vt vin_lds dynamic rec_tsum')


def launch(entry, W, q, d, N, L, mode='path', family='mfma', record=False, xproj=False, max_blocks=0, ngrad=0, want_vt=True,
           vin_lds=True, dynamic=True, rec_tsum=True):
    c = Launch(entry, family, W, q, d, N, L, mode, record, xproj, max_blocks, ngrad, want_vt, vin_lds, dynamic, rec_tsum)
    assert entry in ('fwd', 'bwd', 'gradx') and family in ('mfma', 'tiled') and mode in ('path', 'point')
    assert mode == 'path' or L == 1
    assert 0 <= ngrad <= N * L and (entry != 'gradx' or (L == 1 and not record and not xproj and ngrad == 0))
    assert not xproj or (mode == 'path' and family == 'mfma' and W in CONTAINERS)
    assert entry != 'bwd' or record or (ngrad == 0 and not xproj)       # (disc_bwd alone: no forward of the case's own)
    return c


def cid(c):
    """a case's id: what selects its kernels, then the rest"""
    s = '%s-%s-W%d-q%d-d%d-%s%dx%d' % (c.entry, c.family, c.W, c.q, c.d, c.mode, c.N, c.L)
    s += ('-rec' if c.record else '') + ('-table' if c.xproj else '') + ('-cap%d' % c.max_blocks if c.max_blocks else '')
    s += ('-ngrad%d' % c.ngrad if c.ngrad else '') + ('' if c.want_vt else '-novt')
    return s + ''.join('-%s0' % k for k in SWITCHES if not getattr(c, k))


def switches(c):
    """{environment variable: '0'} of the switches a case turns off"""
    return {ENV[SWITCHES[k]]: '0' for k in SWITCHES if not getattr(c, k)}


def switched_off(c):
    """{option field: False} of the same switches: the arguments of kernels.switched for the case"""
    return {SWITCHES[k]: False for k in SWITCHES if not getattr(c, k)}


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------------
def _nt(W):
    """XWD_DISPATCH: row tiles of the tiled family's kernel"""
    return 4 if W <= 64 else 8 if W <= 128 else 12 if W <= 192 else 16


def _forward(c, N, L, record, xproj, max_blocks):
    """the forward kernel of one disc_fwd call (xw_disc_tiled_fwd / xw_disc_fwd_xproj / the generic fall-through)"""
    if c.family == 'tiled':
        return ('t_fwd', _nt(c.W))
    if c.W not in CONTAINERS:
        return ('g_fwd',)
    ntiles = (N * L + 15) // 16
    blocks = min((ntiles + 3) // 4, max_blocks if max_blocks > 0 else 512)
    dyn = c.dynamic and ntiles > 4 * blocks
    if c.W > 64:                                             # one block per CU: the cap of the wide containers
        blocks = min(blocks, 256)
        dyn = dyn and ntiles > 4 * blocks
    if xproj:
        vks = -1
    elif c.W > 64 or not c.vin_lds:
        vks = 0
    else:
        vks = 6 if (c.d + 3) // 4 <= 6 else 13
    return ('fwd', c.W, bool(record), dyn, vks)


def _reverse(c, N, L):
    """the reverse kernel of one disc_bwd call from a record"""
    if c.family == 'tiled':
        return ('t_bwd', _nt(c.W))
    if c.W not in CONTAINERS:
        return ('g_bwd',)
    ng = 1 if c.d + 2 <= 48 else 2 if c.d + 2 <= 96 else 3
    tsum = c.rec_tsum and c.mode == 'path' and N % 64 == 0
    return ('rec', c.W, 0, ng, tsum)


def _recomputes(c):
    """kernels.disc_recompute: the recomputing reverse kernels exist at the reference's shape only"""
    return c.family == 'mfma' and c.W == 50 and c.q == 9


def reaches(c):
    """the kernel tuples a case lands on, in launch order"""
    ctg = 1 if c.d + 2 <= 64 else 2
    if c.entry == 'gradx':
        if _recomputes(c):
            return [('bwd', 50, 9, ctg, False, True)]
        return [_forward(c, c.N, 1, False, False, 0)]        # the forward's fused gradient at every point (one time index)
    out = []
    if c.entry == 'fwd' or c.record:
        if c.xproj:
            out.append(('xproj',))
        out.append(_forward(c, c.N, c.L, c.record, c.xproj, c.max_blocks))
    if c.entry == 'bwd':
        if c.record:
            out.append(_reverse(c, c.N, c.L))
        elif _recomputes(c):
            out.append(('bwd', 50, 9, ctg, True, False))
        else:                                                # the wrapper stores a record first: default cap, no table
            out += [_forward(c, c.N, c.L, True, False, 0), _reverse(c, c.N, c.L)]
    return out


# ---- the cases: one per compiled kernel at the smallest shape that selects it, then the edges -----------------------------------------
# static split: 15 - 17 points (one or two tiles), default cap; tickets: one block, 65 points = five tiles for four waves, the last
# tile one point
STATIC = ((5, 3), (17, 1))
TICKETS = (13, 5)
VKS_D = {6: (24,), 13: (25, 53, 126), 0: (24, 126), -1: (25, 53)}     # d per input-layer plan (0 at W <= 64: the switch is off)
DEPTHS = (0, 1, 9, 16)


def _forward_cases():
    """every (W, ACT, DYN, VKS): 16 kernels each at W = 50, 64 (8 of them behind XW_DISC_VIN_LDS=0), 8 each at W = 96, 128; the
    modes, depths, ngrad kinds, want_vt and the d values of a plan are spread over them by a running counter"""
    out, k = [], 0                                           # k counts (W, VKS, ACT); the two schedules of a k differ in every spread axis
    for W in CONTAINERS:
        for vks in ((-1, 0, 6, 13) if W <= 64 else (-1, 0)):
            for act in (False, True):
                for dyn in (False, True):
                    kind = (k + dyn) % 4                     # ngrad 0 | 1 | 17 | N: all four with either schedule
                    N, L = TICKETS if dyn else (17, 1) if kind == 2 else STATIC[(k // 4) % 2]
                    d = VKS_D[vks][k % len(VKS_D[vks])]
                    point = vks != -1 and (k + dyn) % 3 == 1
                    if point:
                        N, L = N * L, 1
                    out.append(launch('fwd', W, DEPTHS[(k + 2 * dyn) % 4], d, N, L, mode='point' if point else 'path', record=act,
                                      xproj=vks == -1, max_blocks=1 if dyn else 0, ngrad=(0, 1, 17, N)[kind], want_vt=(k + dyn) % 5 != 4,
                                      vin_lds=not (vks == 0 and W <= 64)))
                k += 1
    return out


def _record_cases():
    """every (W, NG, TSUM): NG by d in {46, 47, 94, 95, 126}, TSUM by (64, 2) / (128, 3) against 17 paths and point mode; the
    corner W = 128, q = 16, d = 126 is among them, with and without TSUM"""
    out, j = [], 0
    for W in CONTAINERS:
        for ng, ds in ((1, (46,)), (2, (47, 94)), (3, (95, 126))):
            corner = W == 128 and ng == 3
            d = 126 if corner else ds[j % len(ds)]
            for tsum in (True, False):
                q = 16 if corner else DEPTHS[(j + tsum) % 4]
                if tsum:
                    N, L = ((64, 2), (128, 3))[j % 2]
                    out.append(launch('bwd', W, q, d, N, L, record=True, ngrad=(0, 64)[(j // 2) % 2]))
                elif j % 2 == 0:
                    out.append(launch('bwd', W, q, d, 17, 3, record=True, ngrad=(17, 1)[(j // 2) % 2]))
                else:
                    out.append(launch('bwd', W, q, d, 17, 1, mode='point', record=True))
            j += 1
    # the other d of the two-valued groups, at the benchmark's width; q = 17 (beyond the fused gradient: family forced, no gxv)
    out += [launch('bwd', 50, 9, 94, 17, 2, record=True), launch('bwd', 50, 1, 95, 64, 2, record=True),
            launch('bwd', 64, 16, 47, 17, 1, mode='point', record=True), launch('bwd', 50, 17, 5, 17, 2, record=True)]
    return out


def _recompute_cases():
    """W = 50, q = 9 without a record: CTG by d in {62, 63, 126}, N in {1, 17, 65}; the parameter gradient and disc_gradx"""
    out = []
    for i, d in enumerate((62, 63, 126)):
        for k, N in enumerate((1, 17, 65)):
            mode = ('path', 'point')[(i + k) % 2]
            out.append(launch('bwd', 50, 9, d, N, 1 if mode == 'point' else (3, 2, 1)[k], mode=mode))
            out.append(launch('gradx', 50, 9, d, N, 1, mode=('point', 'path')[(i + k) % 2]))
    return out


def _tiled_cases():
    return [launch('bwd', W, q, d, N, L, mode=mode, family='tiled', record=True, ngrad=ngrad, max_blocks=1)
            for W, q, d, N, L, mode, ngrad in ((64, 17, 5, 17, 1, 'path', 17), (65, 1, 25, 5, 3, 'path', 1), (129, 9, 53, 17, 1, 'point', 0),
                                               (193, 32, 126, 13, 5, 'path', 13))]


def _generic_cases():
    """any other width up to 128, through the C entry points at W itself: 17 points"""
    out = []
    for i, W in enumerate((1, 17, 49, 51, 127)):
        for k, q in enumerate((0, 1, 16)):
            mode = ('path', 'point')[(i + k) % 2]
            out.append(launch('bwd', W, q, (5, 24, 126, 1, 53)[(i + 2 * k) % 5], 17, 1, mode=mode, record=k != 1,
                              ngrad=(17, 0, 1)[(i + k) % 3] if k != 1 else 0, want_vt=(i + k) % 4 != 3))
    return out


def _edge_cases():
    """what no single kernel needs: disc_bwd / disc_gradx where the wrapper goes through the forward, the rotated static split
    (XW_DISC_DYNAMIC=0 with more tiles than waves: rot = 5 % 4 = 1)"""
    return [launch('bwd', 64, 9, 52, 17, 2), launch('bwd', 96, 1, 5, 15, 1, mode='point'),
            launch('gradx', 64, 4, 25, 17, 1), launch('gradx', 128, 16, 126, 15, 1, mode='point'), launch('gradx', 17, 2, 5, 17, 1),
            launch('gradx', 193, 20, 5, 17, 1, family='tiled'),
            launch('bwd', 50, 9, 24, 13, 5, record=True, max_blocks=1, ngrad=13, dynamic=False),
            launch('bwd', 64, 1, 53, 65, 1, mode='point', record=True, max_blocks=1, ngrad=17, dynamic=False),
            launch('fwd', 96, 4, 5, 13, 5, max_blocks=1, xproj=True, dynamic=False),
            launch('fwd', 50, 16, 126, 13, 5, max_blocks=1, dynamic=False)]


CASES = tuple(_forward_cases() + _record_cases() + _recompute_cases() + _tiled_cases() + _generic_cases() + _edge_cases())
assert len({cid(c) for c in CASES}) == len(CASES)

# a kernel no entry point can select, with the reason (read from the dispatch); empty: every compiled kernel has a case
UNREACHED = {}


def reached():
    """{kernel tuple: [case, ...]} over CASES"""
    out = {}
    for c in CASES:
        for k in reaches(c):
            out.setdefault(k, []).append(c)
    return out


def in_process(c):
    """True for a case that runs under the default switches (the others run inside kernels.switched(**switched_off(c)))"""
    return not switches(c)


if __name__ == '__main__':
    for c_ in CASES:
        print('| %s | %s |' % (cid(c_), ', '.join(repr(k) for k in reaches(c_))))
