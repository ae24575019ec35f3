"""The fused stepper's compiled kernels, and the launch forms that reach them -- TEST INFRASTRUCTURE ONLY (imported like
tests/guarded.py).  CPU only.

The fused stepper (csrc/xw_ode_fwd.h and xw_ode.hip over xw_ode_core.h, the form headers xw_ode_mfma4.h / xw_ode_mfma16.h
and the narrow tiles of xw_ode_n4.h) is compiled once per container, depth, method and launch form: every instantiation is its own
machine code with its own schedule.  Two views of that set:

    compiled(path)      what a built libxnwan.so (or a directory of xw_ode_*.o) holds: the kernel symbols of its gfx950 code objects,
                        names only, parsed to tuples (parse_kernel); code_objects(path): the same, one set per code object
    reaches(H, K, m, method, form)
                        what a launch lands on: a restatement of the selection in csrc/xw_ode_select.h (choose_fwd, choose_sweep,
                        recomp_slot) and of the tables its slots index (xw_ode_fwd.h, xw_ode.hip), in terms of what a caller
                        of kernels.ode_fwd_multi / ode_bwd_multi passes

tests/test_stepper_inventory_host.py asserts that the two are the same set; tests/test_gpu_stepper_inventory.py runs every form of
every case against the oracle, so a new instantiation cannot appear without a case that runs it.

Kernel tuples:   ('fwd', H, K, M, METHOD, ACT)                   k_ode_fwd         ACT 0 no store, 1 full store, 2 x-only store
                 ('fwd_n4', H, K, M, METHOD, ACT)                n4::k_ode_fwd_n4
                 ('bwd', H, K, M, METHOD, PARAMS, SAVED, ADJ)    k_ode_bwd         SAVED: from the activation store
                 ('bwd_duo', H, K, M, METHOD)                    k_ode_bwd_duo
                 ('bwd_n4', H, K, M, METHOD, PARAMS)             n4::k_ode_bwd_n4
"""
import importlib.util
import os
import re
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tools/isa_same.py, loaded by path: sys.path stays as it is and no bare top-level name 'isa_same' appears for the other tests
_spec = importlib.util.spec_from_file_location('_xw_tools_isa_same', os.path.join(ROOT, 'tools', 'isa_same.py'))
isa_same = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_same)

METHODS = ('euler', 'midpoint', 'rk4')                       # method ids 0, 1, 2 (kernels.METHODS)
ODE_WIDTHS = ((20, 10), (32, 12), (64, 16))                  # kernels.ODE_WIDTHS (asserted by the host test)
NARROW_WIDTHS = ((20, 10), (32, 12))                         # the 4x4x4 containers: the only ones with narrow tiles (XW_ODE_HAS_NARROW)
DEPTHS = tuple(range(1, 11))                                 # XW_ODE_DEPTHS of xw_ode_select.h.  Nothing reads it: what binds DEPTHS (and the
                                                             # two tuples above, beyond the host test's comparison with `kernels`) to the
                                                             # build is the set equality reaches == compiled of the host test

FAMILIES = {'k_ode_fwd': 'fwd', 'k_ode_fwd_n4': 'fwd_n4', 'k_ode_bwd': 'bwd', 'k_ode_bwd_duo': 'bwd_duo', 'k_ode_bwd_n4': 'bwd_n4'}
_ARGS = {'fwd': 5, 'fwd_n4': 5, 'bwd': 7, 'bwd_duo': 4, 'bwd_n4': 5}
_NAME = re.compile(r'(?<![\w])(k_ode_fwd_n4|k_ode_bwd_n4|k_ode_bwd_duo|k_ode_fwd|k_ode_bwd)<([^<>]*)>\(')


def parse_kernel(text):
    """the kernel tuple of a demangled name as llvm-objdump and rocprofv3 spell it ('void (anonymous namespace)::k_ode_fwd<20, 10,
    8, 1, 2>((anonymous namespace)::FwdJobs, ...)'); None if `text` names no stepper kernel"""
    m = _NAME.search(text)
    if m is None:
        return None
    family = FAMILIES[m.group(1)]
    args = tuple({'true': True, 'false': False}[a] if a in ('true', 'false') else int(a) for a in (s.strip() for s in m.group(2).split(',')))
    if family == 'bwd' and len(args) == 6:
        args += (False,)                                     # (ADJ's default, should a demangler leave it out)
    assert len(args) == _ARGS[family], text
    return (family,) + args


def code_objects(path):
    """the stepper kernel tuples of `path` (a libxnwan.so, one object, or a directory of xw_ode_*.o), one set per gfx950 code object
    that holds any.  Reads the function symbols of .text (llvm-objdump -t --demangle); never an instruction."""
    files = sorted(os.path.join(path, n) for n in os.listdir(path) if re.match(r'xw_ode_.*\.o$', n)) if os.path.isdir(path) else [path]
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for f in files:
            for co in isa_same.bundles(f, tmp):
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
    """the set of stepper kernel tuples in `path`, over all its code objects"""
    found = set()
    for obj in code_objects(path):
        assert not found & obj, 'compiled twice: %r' % sorted(found & obj, key=repr)
        found |= obj
    return found


# ---- launch forms ------------------------------------------------------------------------------------------------------------------
# forward: what kernels.ode_fwd_multi is given.  store: None (no 'act' in the job), 'full', 'x' (act_x_only=True)
FWD_FORMS = {
    'fwd':           dict(store=None, narrow=False),
    'fwd_store':     dict(store='full', narrow=False),
    'fwd_xstore':    dict(store='x', narrow=False),
    'fwd_n4':        dict(store=None, narrow=True),
    'fwd_n4_store':  dict(store='full', narrow=True),
    'fwd_n4_xstore': dict(store='x', narrow=True),
}
# sweeps: what kernels.ode_bwd_multi is given.  producer: the forward form whose Y (and store, if it has one) the job carries
BWD_FORMS = {
    'x_from_store':  dict(producer='fwd_store', params=False, adjoint=False, narrow=False),
    'x_from_xstore': dict(producer='fwd_xstore', params=False, adjoint=False, narrow=False),      # the same kernel, the second producer
    'duo':           dict(producer='fwd_store', params=True, adjoint=False, narrow=False),
    'recomp_x':      dict(producer='fwd', params=False, adjoint=False, narrow=False),
    'recomp_w':      dict(producer='fwd', params=True, adjoint=False, narrow=False),
    'adjoint_x':     dict(producer='fwd', params=False, adjoint=True, narrow=False),
    'adjoint_w':     dict(producer='fwd', params=True, adjoint=True, narrow=False),
    'n4_x':          dict(producer='fwd_n4_store', params=False, adjoint=False, narrow=True),
    'n4_w':          dict(producer='fwd_n4_store', params=True, adjoint=False, narrow=True),
}
FORMS = tuple(FWD_FORMS) + tuple(BWD_FORMS)


def forms_of(H, K, m, method):
    """the forms that exist for a case (the same at every depth today: m is part of the case, not of the rule).  rk4 keeps no activation store (xw_ode_act_rows is 0, the entry points drop the pointer), so
    it has the forms without one; narrow tiles exist in the 4x4x4 containers only (at (64, 16) a launch that asks for them runs the
    16-path kernels, which the other forms already reach)."""
    out = []
    for f in FORMS:
        spec = FWD_FORMS.get(f) or BWD_FORMS[f]
        store = FWD_FORMS[spec['producer']]['store'] if f in BWD_FORMS else spec['store']
        narrow = spec['narrow'] or (f in BWD_FORMS and FWD_FORMS[spec['producer']]['narrow'])
        if store is not None and method == 'rk4':
            continue
        if narrow and (H, K) not in NARROW_WIDTHS:
            continue
        out.append(f)
    return out


def reaches(H, K, m, method, form):
    """the kernel tuple that `form` lands on at (H, K, m, method); KeyError if the case has no such form"""
    if form not in forms_of(H, K, m, method):
        raise KeyError((H, K, m, method, form))
    mid = METHODS.index(method)
    if form in FWD_FORMS:
        # choose_fwd: method * 3 + (0 no store, 1 full, 2 x-only) of the seven forward kinds; the narrow-tile kernel of the same kind
        # when the jobs ask for narrow tiles
        spec = FWD_FORMS[form]
        return ('fwd_n4' if spec['narrow'] else 'fwd', H, K, m, mid, {None: 0, 'full': 1, 'x': 2}[spec['store']])
    spec = BWD_FORMS[form]
    if spec['narrow']:                                       # choose_sweep: narrow first, from the store only
        return ('bwd_n4', H, K, m, mid, spec['params'])
    store = FWD_FORMS[spec['producer']]['store'] is not None
    if spec['adjoint'] or not store or mid > 1:              # SWEEP_RECOMP, recomp_slot: k_ode_bwd<.., PARAMS, false, ADJ>
        return ('bwd', H, K, m, mid, spec['params'], False, spec['adjoint'])
    if spec['params']:
        return ('bwd_duo', H, K, m, mid)
    return ('bwd', H, K, m, mid, False, True, False)


CASES = tuple((H, K, m, method) for H, K in ODE_WIDTHS for m in DEPTHS for method in METHODS)


def reached():
    """{kernel tuple: [(case, form), ...]} over every form of every case"""
    out = {}
    for c in CASES:
        for f in forms_of(*c):
            out.setdefault(reaches(*c, f), []).append((c, f))
    return out
