"""Tensor-level wrappers around the C ABI: every operand is validated on the host (device, dtype, contiguity,
shape) BEFORE a kernel is enqueued, then passed as a raw device pointer together with torch's current stream.

Conventions (include/xnwan.h): point arrays are time-major [L, N]; coordinates are transposed xT[d, N]; all float64.
"""
import contextlib
import ctypes
import dataclasses
import types

import torch

from ._lib import (lib, check, XnwanError, XwOdeFwdJob, XwOdeBwdJob, XwDopriJob, XwDopriSweepJob, XwPathsJob, XwPathsDopriJob,
                   XwPathsGradJob, XwPathsHvpJob, XwPathsJetJob, XwPathsVjpJob, XwPathsGvjpJob, XwPathsDopriCkptJob, XwPathsDopriGradJob, XwSwitches)
from .options import EngineOptions

METHODS = {'euler': 0, 'midpoint': 1, 'rk4': 2}
DOPRI5 = 3                                 # solver 'dopri5' (adaptive, dopri5_fwd / dopri5_sweep below): not a fixed-grid method id
ADAMS = 4                                  # solver 'explicit_adams' (fixed-grid Adams-Bashforth): the tiled family only (adams_tiled_* below)
ADAPTIVE_REFUSED = ('dopri8', 'bosh3', 'fehlberg2', 'adaptive_heun', 'adams', 'implicit_adams',
                    'fixed_adams', 'scipy_solver')   # torchdiffeq's other methods: not served
F32, F64 = torch.float32, torch.float64


def _need_gpu():
    if not torch.cuda.is_available():
        raise XnwanError('no GPU visible: the XNODE-WAN kernels only run on an MI355X (gfx950); there is no CPU path')


# Operand validation costs ~0.7 us per check and a list-domain outer iteration makes ~28 000 of them (1.9 ms of its ~23).  The
# engine's own buffers are allocated by the engine with exactly these shapes: while TRUSTED is set (engine.Engine sets it
# around the eager sub-steps of list-domain groups, whose launches are issued from Python one by one) the checks are skipped.
# Everything reachable from user code -- the module call surface, the custom operators, the first launch of every captured
# graph -- stays checked.
TRUSTED = False


# ---- the library switches (options.py: the last block of EngineOptions; include/xnwan_switches.h) --------------------------------
LIB_SWITCHES = tuple(name for name, _ in XwSwitches._fields_)     # the six the C library holds; lone_narrow is ode_fwd's, below
_lone_narrow = True


def apply_switches(opt):
    """set the process-wide switches from `opt` (an EngineOptions, or anything with the seven fields); the last call wins"""
    global _lone_narrow
    sw = XwSwitches(*(int(getattr(opt, name)) for name in LIB_SWITCHES))
    check(lib.xw_switches_set(ctypes.byref(sw)), 'xw_switches_set')
    _lone_narrow = bool(opt.lone_narrow)


def switches():
    """{field: value} of the seven as they stand, the library's six read back from the library"""
    sw = XwSwitches()
    check(lib.xw_switches_get(ctypes.byref(sw)), 'xw_switches_get')
    kinds = {f.name: f.type for f in dataclasses.fields(EngineOptions)}       # (bool for the flags, int for the two numbers)
    out = {name: kinds[name](getattr(sw, name)) for name in LIB_SWITCHES}
    out['lone_narrow'] = _lone_narrow
    return out


@contextlib.contextmanager
def switched(**fields):
    """`with switched(duo_spread=False): ...` -- the named switches changed for the block, the previous values back behind it"""
    before = switches()
    unknown = set(fields) - set(before)
    if unknown:
        raise TypeError('not a library switch: %s' % sorted(unknown))
    apply_switches(types.SimpleNamespace(**dict(before, **fields)))
    try:
        yield
    finally:
        apply_switches(types.SimpleNamespace(**before))


apply_switches(EngineOptions.from_env())


def _chk(t, dtype, shape, name):
    if t is None or TRUSTED:
        return
    if not (torch.is_tensor(t) and t.is_cuda):
        raise XnwanError('%s must be a CUDA/HIP tensor' % name)
    if t.dtype != dtype:
        raise XnwanError('%s must be %s, got %s' % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise XnwanError('%s must be contiguous' % name)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise XnwanError('%s must have shape %s, got %s' % (name, tuple(shape), tuple(t.shape)))


def _p(t):
    return 0 if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream():
    """raw handle of torch's current stream on the current device (the C call: no Stream object per launch -- a list
    domain issues ~500 launches per outer iteration from Python)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def method_id(name):
    if name == 'dopri5':
        return DOPRI5
    if name == 'explicit_adams':
        return ADAMS
    if name not in METHODS:
        raise XnwanError("solver %r is not served: the fixed-grid schemes %s, the fixed-grid Adams-Bashforth 'explicit_adams' and the "
                         "adaptive 'dopri5' are (no other adaptive torchdiffeq method, no predictor-corrector Adams)" % (name, sorted(METHODS)))
    return METHODS[name]


# Kernel instantiations (the tables of csrc/xw_ode_fwd.h and xw_ode.hip, csrc/xw_disc_fwd.hip, xw_disc_rec.hip, xw_disc_bwd.hip): widths the MFMA kernels are compiled for.  Any
# smaller network runs EXACTLY inside the next larger instantiation: its parameters are embedded in a zero-padded blob
# (nets.Blob) -- padding units have zero in- and outgoing weights and zero bias, so they stay identically zero through
# relu / tanh, contribute exact zeros to every sum, and receive exactly zero gradients (Adam leaves them at zero).
# Anything wider runs, at its own widths, on the GENERIC path (csrc/xw_generic.hip: per-path / per-point code on the vector ALU,
# two to three orders of magnitude slower -- there so that every legal configuration of the reference trains).
ODE_WIDTHS = [(20, 10), (32, 12), (64, 16)]   # (u_hidden_dim, u_hidden_hidden_dim) containers, smallest first.  (64, 16) (round 6) is the
                                           # WIDE container: the field on 16x16x4 matrix instructions, one wave per tile (+ a partner in the sweep with weight gradients), depths 1..10
                                           # (deeper fields: the generic path, at the network's own widths)
DISC_WIDTHS = [50, 64, 96, 128]            # v_hidden_dim containers (W = 50: 3 MFMA row tiles + a 2-row vector tail; 64: 4 tiles;
                                           # 96, 128 (round 6): 6 / 8 tiles, one block per CU, forward + reverse from the record)
GENERIC_ODE_MAX = (64, 16)                 # csrc/xw_generic.h
GENERIC_DISC_MAX = 128


ODE_WIDE_MAX_DEPTH = 10                    # (64, 16): 4 (u_layers - 1) ReLU-mask bits per stage, two words at depth 10
ODE_MAX_DEPTH = 10                         # the other containers (csrc/xw_common.h XW_ODE_MAX_LAYERS); deeper fields, up to
GENERIC_ODE_MAX_DEPTH = 32                 # this (csrc/xw_generic.h XWG_MAX_M), run on the generic path at their own widths


def ode_container(H, K, m=1):
    """the widths the stepper kernels run a (u_hidden_dim H, u_hidden_hidden_dim K) network of u_layers = m at"""
    for Hc, Kc in ODE_WIDTHS:
        if m > (ODE_WIDE_MAX_DEPTH if (Hc, Kc) == ODE_WIDTHS[-1] else ODE_MAX_DEPTH):
            continue                       # (u_layers > 10: the generic path, at the network's own widths)
        if H <= Hc and K <= Kc and lib.xw_theta_size(1, Hc, Kc) > 0 and lib.xw_ode_act_rows(0, Hc, Kc, 1) >= 0:
            return Hc, Kc
    if H <= GENERIC_ODE_MAX[0] and K <= GENERIC_ODE_MAX[1] and m <= GENERIC_ODE_MAX_DEPTH and lib.xw_ode_act_rows(0, H, K, m) >= 0:
        return H, K                        # the generic path, at the network's own widths
    raise XnwanError('u_hidden_dim = %d, u_hidden_hidden_dim = %d, u_layers = %d: the stepper kernels serve widths up to %s (MFMA) / %s (generic '
                     'path), depths up to %d / %d' % (H, K, m, ODE_WIDTHS[-1], GENERIC_ODE_MAX, ODE_MAX_DEPTH, GENERIC_ODE_MAX_DEPTH))


def ode_generic(H, K, m=1):
    """True when (H, K) at u_layers = m is served by the generic (slow) path rather than by an MFMA instantiation"""
    return (H, K) not in ODE_WIDTHS or m > (ODE_WIDE_MAX_DEPTH if (H, K) == ODE_WIDTHS[-1] else ODE_MAX_DEPTH)


TILED_ODE_MAX = (256, 256)                 # csrc/xw_tiled.hip: the tiled family, at the network's own widths, depths up to
TILED_ODE_MAX_DEPTH = 32                   # this, fixed-grid methods only
TILED_POLICIES = ('beyond', 'generic')     # EngineOptions.tiled_stepper


def stepper_family(H, K, m=1, policy='beyond', method=None):
    """which stepper family runs a (u_hidden_dim H, u_hidden_hidden_dim K, u_layers m) field: 'mfma' (the fused containers),
    'generic' (csrc/xw_generic.hip) or 'tiled' (csrc/xw_tiled.hip).  policy 'beyond': the tiled family only where the other two
    refuse; 'generic': also in place of the generic path.  method == ADAMS (explicit_adams): the tiled family at every width it
    serves -- the only family with that solver."""
    if policy not in TILED_POLICIES:
        raise XnwanError('tiled_stepper = %r: one of %s' % (policy, TILED_POLICIES))
    if not (1 <= H <= TILED_ODE_MAX[0] and 1 <= K <= TILED_ODE_MAX[1] and 1 <= m <= TILED_ODE_MAX_DEPTH):
        raise XnwanError('u_hidden_dim = %d, u_hidden_hidden_dim = %d, u_layers = %d: the stepper kernels serve widths up to %s (MFMA) / '
                         '%s (generic path) / %s (tiled), depths up to %d / %d / %d'
                         % (H, K, m, ODE_WIDTHS[-1], GENERIC_ODE_MAX, TILED_ODE_MAX, ODE_MAX_DEPTH, GENERIC_ODE_MAX_DEPTH, TILED_ODE_MAX_DEPTH))
    if method == ADAMS:
        return 'tiled'
    try:
        Hc, Kc = ode_container(H, K, m)
    except XnwanError:
        return 'tiled'
    if not ode_generic(Hc, Kc, m):
        return 'mfma'
    return 'tiled' if policy == 'generic' else 'generic'


def stepper_kdims(H, K, m=1, policy='beyond', method=None):
    """the widths the parameter blob is laid out at: the MFMA container, or the network's own (generic, tiled)"""
    return ode_container(H, K, m) if stepper_family(H, K, m, policy, method) != 'tiled' else (H, K)


def disc_container(W):
    for Wc in DISC_WIDTHS:
        if W <= Wc and lib.xw_disc_act_rows(Wc, 1) >= 0:
            return Wc
    if W <= GENERIC_DISC_MAX and lib.xw_disc_act_rows(W, 1) >= 0:
        return W
    raise XnwanError('v_hidden_dim = %d: the test-network kernels serve widths up to %d (MFMA) / %d (generic path)'
                     % (W, DISC_WIDTHS[-1], GENERIC_DISC_MAX))


def disc_generic(W):
    return W not in DISC_WIDTHS


TILED_DISC_MAX = 256                       # csrc/xw_disc_tiled.hip: the tiled test-network family, at the network's own width,
TILED_DISC_MAX_DEPTH = 32                  # v_layers up to this
DISC_MAX_GRAD_DEPTH = 16                   # deepest test network the MFMA entry points run with the fused input gradient
TESTNET_FAMILIES = ('mfma', 'tiled')


def testnet_family(W, q):
    """which family runs a (v_hidden_dim W, v_layers q) test network: 'mfma' (today's C entry points xw_disc_*: the MFMA containers
    and, between them, the generic path) for W <= 128 and q <= 16, 'tiled' (csrc/xw_disc_tiled.hip) for the rest up to 256 / 32"""
    if not (1 <= W <= TILED_DISC_MAX and 0 <= q <= TILED_DISC_MAX_DEPTH):
        raise XnwanError('v_hidden_dim = %d, v_layers = %d: the test-network kernels serve widths up to %d (MFMA containers %s) / %d '
                         '(generic path) / %d (tiled), depths up to %d / %d / %d'
                         % (W, q, DISC_WIDTHS[-1], DISC_WIDTHS, GENERIC_DISC_MAX, TILED_DISC_MAX, DISC_MAX_GRAD_DEPTH,
                            DISC_MAX_GRAD_DEPTH, TILED_DISC_MAX_DEPTH))
    return 'mfma' if W <= GENERIC_DISC_MAX and q <= DISC_MAX_GRAD_DEPTH else 'tiled'


def testnet_kwidth(W, q):
    """the width the test network's parameter blob is laid out at: the container ('mfma'), the network's own ('tiled')"""
    return disc_container(W) if testnet_family(W, q) == 'mfma' else W


def _disc_family(W, q, family):
    if family is None:
        return testnet_family(W, q)
    if family not in TESTNET_FAMILIES:
        raise XnwanError('family = %r: one of %s' % (family, TESTNET_FAMILIES))
    return family


def theta_size(d, H, K):
    return lib.xw_theta_size(d, H, K)


def phi_size(d, W):
    return lib.xw_phi_size(d, W)


def ode_fwd(xT, t, start, theta, method, H, K, m, want_Y=True, u=None, Y=None):
    """u_theta on N paths: returns (u[L,N], Y[L,H,N] or None)."""
    _need_gpu()
    d, N = xT.shape
    L = t.shape[0]
    _chk(xT, F64, (d, N), 'xT'); _chk(t, F64, (L,), 't'); _chk(start, F64, (N,), 'start')
    _chk(theta, F64, (theta_size(d, H, K),), 'theta')
    if u is None:
        u = torch.empty(L, N, dtype=F64, device=xT.device)
    if Y is None and want_Y:
        Y = torch.empty(L, H, N, dtype=F64, device=xT.device)
    _chk(u, F64, (L, N), 'u'); _chk(Y, F64, (L, H, N), 'Y')
    if Y is None and _lone_narrow and (N + 15) // 16 <= 256 and (H, K) in ODE_WIDTHS:
        # an evaluation on its own (the diagnostic, a stop hook, Engine.predict) has the chip to itself: up to 256 tiles the narrow
        # layout -- four waves of 4 paths per tile, every SIMD busy -- ends sooner (57 against 73 us at 4096 paths x 32 times,
        # 109 against 143 at 64 times; beyond 256 tiles it loses: tools/lone_forward.py).  Same values to the last bit or two.
        arr = (XwOdeFwdJob * 1)()
        _fwd_job(arr[0], dict(xT=xT, start=start, u=u), d, L, H, narrow=True)
        check(lib.xw_ode_fwd_multi(arr, 1, _p(t), _p(theta), method, L, d, H, K, m, 0, _stream()), 'xw_ode_fwd_multi')
        return u, None
    check(lib.xw_ode_fwd(_p(xT), _p(t), _p(start), _p(theta), method, N, L, d, H, K, m, _p(u), _p(Y), _stream()), 'xw_ode_fwd')
    return u, Y


def _launch_dims(jobs, t, theta, H, K):
    """(L, d, P_u) of a launch over `jobs`, with t and theta checked against them"""
    L, d = t.shape[0], jobs[0]['xT'].shape[0]
    P = theta_size(d, H, K)
    _chk(t, F64, (L,), 't'); _chk(theta, F64, (P,), 'theta')
    return L, d, P


def _act(j, store, L, H, N):
    """a job's activation store, checked, where the family keeps one (store = (method, K, m): the fused and generic paths), else None"""
    act = j.get('act') if store is not None else None
    if act is not None:
        _chk(act, F64, (max(L - 1, 1), ode_act_rows(store[0], H, store[1], store[2]), ode_act_cols(N)), 'act')
    return act


def _fwd_job(a, j, d, L, H, store=None, act_x_only=False, narrow=False, prio_drop=0, hints=True):
    """check one forward job (dict of xT[d,N], start[N], u[L,N], Y[L,H,N] or None) against the launch's (d, L, H) and fill `a`; returns
    N.  store: _act's; hints=False: `a` is an XwDopriJob, which has none of act / act_x_only / narrow / prio_drop"""
    N = j['xT'].shape[1]
    _chk(j['xT'], F64, (d, N), 'xT'); _chk(j['start'], F64, (N,), 'start'); _chk(j['u'], F64, (L, N), 'u')
    _chk(j.get('Y'), F64, (L, H, N), 'Y')
    a.xT, a.start, a.u, a.Y, a.N = _p(j['xT']), _p(j['start']), _p(j['u']), _p(j.get('Y')), N
    if hints:
        a.act, a.act_x_only, a.narrow, a.prio_drop = _p(_act(j, store, L, H, N)), 1 if act_x_only else 0, 1 if narrow else 0, int(prio_drop)
    return N


def ode_fwd_multi(jobs, t, theta, method, H, K, m, zero16=None, act_x_only=False, narrow=False, prio_drop=0):
    """jobs: list of dicts(xT[d,N], start[N], u[L,N], Y[L,H,N] or None) -- all groups share t, theta; ONE launch.
    act_x_only: the activation stores of this launch will only be read by sweeps without weight gradients (the
    discriminator sub-step): only the tanh rows and the ReLU-mask words are written.
    narrow: narrow tiles (XwOdeFwdJob.narrow, csrc/xw_ode_n4.h): four waves of 4 paths per 16-path tile -- same outputs, same
    store; for launches that leave SIMDs idle."""
    _need_gpu()
    L, d, _ = _launch_dims(jobs, t, theta, H, K)
    arr = (XwOdeFwdJob * len(jobs))()
    for a, j in zip(arr, jobs):
        _fwd_job(a, j, d, L, H, (method, K, m), act_x_only, narrow, prio_drop)
    _chk(zero16, F64, (16,), 'zero16')
    check(lib.xw_ode_fwd_multi(arr, len(jobs), _p(t), _p(theta), method, L, d, H, K, m, _p(zero16), _stream()), 'xw_ode_fwd_multi')


def _set_res(a, j, L, N):
    res = j.get('res')
    if res is not None:
        # cotangent formed from a residual inside the sweep (XwOdeBwdJob.res_*): base + coef (u - ref)
        if j.get('ubar') is not None:
            raise XnwanError('a sweep job takes a stored cotangent (ubar) or a residual (res), not both')
        if res.get('weak') is not None:
            # the weak form's dI/du: coef d(c(u) u)/du v w (+ base v at the last time index); ref = v
            wk = res['weak']
            wpp = wk['w'].dim() == 2
            _chk(res['u'], F64, (L, N), 'res.u'); _chk(res['ref'], F64, (L, N), 'res.ref (v)')
            _chk(wk['w'], F64, (L, N) if wpp else (N,), 'res.weak.w'); _chk(wk.get('c'), F64, (L, N), 'res.weak.c')
            _chk(wk.get('cp'), F64, (L, N), 'res.weak.cp')
            a.res_first_only, a.res_u, a.res_ref = 2, _p(res['u']), _p(res['ref'])
            a.res_w_per_point, a.res_w, a.res_c, a.res_cp = int(wpp), _p(wk['w']), _p(wk.get('c')), _p(wk.get('cp'))
            a.res_kappa2 = 2.0 * float(wk.get('ckappa', 0.0))
            mg = res.get('merged')
            if mg is not None:
                # kind 3: [base_A + coef_A (u - ref_A) at l = 0] + (2 / scal[0]) (the weak form above) -- one interior sweep for
                # the generator's cotangents A and B once I = scal[0] is on the device (XwOdeBwdJob.res_first_only == 3)
                _chk(mg.get('ref'), F64, (N,), 'res.merged.ref'); _chk(mg.get('scal'), F64, None, 'res.merged.scal')
                a.res_first_only, a.res_scal, a.res_refA = 3, _p(mg.get('scal')), _p(mg.get('ref'))
                a.res_coefA, a.res_baseA = float(mg['coef']), float(mg['base'])
        else:
            first = bool(res['first_only'])
            _chk(res['u'], F64, (L, N), 'res.u'); _chk(res['ref'], F64, (N,) if first else (L, N), 'res.ref')
            a.res_first_only, a.res_u, a.res_ref = int(first), _p(res['u']), _p(res['ref'])
        a.res_coef, a.res_base = float(res['coef']), float(res['base'])


def _sweep_job(b, j, d, L, H, P, want_x, want_params, x_cot_ones, slabs, with_Y=True, store=None):
    """check one sweep job (ode_bwd_multi's dict) against the launch's (d, L, H, P) and fill b, an XwOdeBwdJob (dopri5: the .b of its
    job), residual fields included.  slabs(N): the family's slab count; with_Y=False: dopri5 reverses its record, Y = 0; store: _act's"""
    N = j['xT'].shape[1]
    Y = j['Y'] if with_Y else None
    _chk(j['xT'], F64, (d, N), 'xT'); _chk(j['start'], F64, (N,), 'start'); _chk(Y, F64, (L, H, N), 'Y')
    _chk(j.get('ubar'), F64, (L, N), 'ubar')
    if want_x and not (x_cot_ones and j.get('gx') is None):
        _chk(j['gx'], F64, (d, N), 'gx'); _chk(j['gs'], F64, (N,), 'gs')
    if want_params:
        _chk(j['gslab'], F64, (slabs(N), P), 'gslab')
    b.xT, b.start, b.Y, b.act, b.ubar, b.N = _p(j['xT']), _p(j['start']), _p(Y), _p(_act(j, store, L, H, N)), _p(j.get('ubar')), N
    b.gx, b.gs, b.gslab = _p(j.get('gx')), _p(j.get('gs')), _p(j.get('gslab'))
    _set_res(b, j, L, N)


def _mode_word(want_x, want_params, x_cot_ones=False, adjoint=False, narrow=False, prio_drop=0):
    """the sweeps' `mode` argument (include/xnwan.h)"""
    return ((1 if want_x else 0) | (2 if want_params else 0) | (4 if x_cot_ones else 0) | (8 if adjoint else 0)
            | (16 if narrow else 0) | ((int(prio_drop) & 3) << 5))


def ode_bwd_multi(jobs, t, theta, method, H, K, m, want_x, want_params, x_cot_ones=False, adjoint=False, narrow=False, prio_drop=0):
    """jobs: list of dicts(xT, start, Y, ubar or None, gx, gs, gslab); ONE launch for all groups.
    res = dict(u[L,N], ref ([N] with first_only, else [L,N]), coef, base, first_only) instead of ubar: the cotangent
    base + coef (u - ref) (at l = 0 only with first_only) is formed inside the sweep.
    res = dict(u, ref=v, coef, base, weak=dict(w, c, cp, ckappa)): the weak form's dI/du; with merged=dict(ref=h[N], coef, base,
    scal[16]) on top: (the first_only form of `merged`) + (2 / scal[0]) dI/du, the generator's two interior sweeps as one.
    x_cot_ones (with want_x and want_params): gx, gs for the all-ones cotangent, parameter gradients for ubar, which must
    equal 1 at every time index >= 1; jobs without gx / gs produce no x outputs.
    adjoint: the continuous adjoint of torchdiffeq.odeint_adjoint (config['adjoint'] = True) instead of the reverse of
    the steps taken; ignores the activation store.
    narrow: narrow tiles (mode bit 4, csrc/xw_ode_n4.h): four waves of 4 paths per 16-path tile instead of one -- for
    launches that leave SIMDs idle; needs every job's activation store (euler, midpoint)."""
    _need_gpu()
    L, d, P = _launch_dims(jobs, t, theta, H, K)
    arr = (XwOdeBwdJob * len(jobs))()
    for a, j in zip(arr, jobs):
        _sweep_job(a, j, d, L, H, P, want_x, want_params, x_cot_ones, ode_bwd_slabs, store=(method, K, m))
    if x_cot_ones and not (want_x and want_params):
        raise XnwanError('x_cot_ones needs want_x and want_params')
    if x_cot_ones and adjoint:
        raise XnwanError('x_cot_ones is not available with the continuous adjoint')
    if narrow and (adjoint or method > 1 or any(j.get('act') is None for j in jobs)):
        raise XnwanError('narrow-tile sweeps run from the activation store of euler / midpoint (no adjoint=True, no rk4)')
    mode = _mode_word(want_x, want_params, x_cot_ones, adjoint, narrow, prio_drop)
    check(lib.xw_ode_bwd_multi(arr, len(jobs), _p(t), _p(theta), method, L, d, H, K, m, mode, _stream()), 'xw_ode_bwd_multi')


def tiled_ode_work(sweep, d, H, K, m, tiles, dev, method=None):
    """the workspace of one tiled launch over `tiles` 16-path tiles (csrc/xw_tiled.hip: per-tile vectors; explicit_adams: and
    its history)"""
    per = (lib.xw_adams_tiled_work if method == ADAMS else lib.xw_tiled_ode_work)(1 if sweep else 0, d, H, K, m)
    check(min(per, 0), 'xw_tiled_ode_work')
    return torch.empty(per * tiles, dtype=F64, device=dev)


def tiled_ode_fwd_multi(jobs, t, theta, method, H, K, m, zero16=None, prio_drop=0, **_hints):
    """ode_fwd_multi on the tiled family (csrc/xw_tiled.hip): jobs as there (act, act_x_only and narrow are hints the family
    does not take: no activation store, no narrow tiles); theta at the network's own widths.  method ADAMS: adams_tiled_fwd_multi"""
    if method == ADAMS:
        return adams_tiled_fwd_multi(jobs, t, theta, H, K, m, zero16=zero16, prio_drop=prio_drop)
    _tiled_fwd(jobs, t, theta, method, H, K, m, zero16, prio_drop)


def adams_tiled_fwd_multi(jobs, t, theta, H, K, m, zero16=None, prio_drop=0, **_hints):
    """solver 'explicit_adams' forward on the tiled family (xw_adams_tiled_fwd_multi): jobs, outputs and widths as
    tiled_ode_fwd_multi"""
    _tiled_fwd(jobs, t, theta, ADAMS, H, K, m, zero16, prio_drop)


def _tiled_fwd(jobs, t, theta, method, H, K, m, zero16, prio_drop):
    _need_gpu()
    L, d, _ = _launch_dims(jobs, t, theta, H, K)
    if method != ADAMS and method not in METHODS.values():
        raise XnwanError("the tiled stepper family runs the fixed-grid methods %s and 'explicit_adams' only" % sorted(METHODS))
    arr = (XwOdeFwdJob * len(jobs))()
    for a, j in zip(arr, jobs):
        _fwd_job(a, j, d, L, H, prio_drop=prio_drop)
    _chk(zero16, F64, (16,), 'zero16')
    work = tiled_ode_work(False, d, H, K, m, sum(lib.xw_tiled_ode_bwd_slabs(a.N) for a in arr), t.device, method)
    entry, sel = ('xw_adams_tiled_fwd_multi', ()) if method == ADAMS else ('xw_tiled_ode_fwd_multi', (method,))   # (Adams takes no method id)
    check(getattr(lib, entry)(arr, len(jobs), _p(t), _p(theta), *sel, L, d, H, K, m, _p(zero16), _p(work), _stream()), entry)


def tiled_ode_bwd_multi(jobs, t, theta, method, H, K, m, want_x, want_params, x_cot_ones=False, adjoint=False, narrow=False,
                        prio_drop=0):
    """ode_bwd_multi on the tiled family: the same jobs (stored cotangent or residual form), outputs and slab format; the sweep
    recomputes from the checkpoints Y.  No continuous adjoint, no narrow tiles.  method ADAMS: adams_tiled_bwd_multi"""
    if method == ADAMS:
        return adams_tiled_bwd_multi(jobs, t, theta, H, K, m, want_x, want_params, x_cot_ones=x_cot_ones, adjoint=adjoint,
                                     narrow=narrow, prio_drop=prio_drop)
    _tiled_bwd(jobs, t, theta, method, H, K, m, want_x, want_params, x_cot_ones, adjoint, narrow, prio_drop)


def adams_tiled_bwd_multi(jobs, t, theta, H, K, m, want_x, want_params, x_cot_ones=False, adjoint=False, narrow=False, prio_drop=0):
    """solver 'explicit_adams' sweep on the tiled family (xw_adams_tiled_bwd_multi): jobs, cotangent forms, outputs and slab
    format as tiled_ode_bwd_multi; step sizes are constants of the reverse pass"""
    if adjoint:
        raise XnwanError("solver 'explicit_adams' with adjoint=True (the continuous adjoint) is not served: its sweep reverses the "
                         "Adams-Bashforth recurrence (u_hidden_dim = %d, u_hidden_hidden_dim = %d)" % (H, K))
    _tiled_bwd(jobs, t, theta, ADAMS, H, K, m, want_x, want_params, x_cot_ones, adjoint, narrow, prio_drop)


def _tiled_adjoint_refused(H, K, m=None):      # (m: the single-group call surface names u_layers in place of the reason)
    return XnwanError('adjoint=True (the continuous adjoint) is not served by the tiled stepper family (u_hidden_dim = %d, '
                      'u_hidden_hidden_dim = %d%s' % (H, K, '): it reverses the steps taken' if m is None else ', u_layers = %d)' % m))


def _tiled_bwd(jobs, t, theta, method, H, K, m, want_x, want_params, x_cot_ones, adjoint, narrow, prio_drop):
    _need_gpu()
    if adjoint:
        raise _tiled_adjoint_refused(H, K)
    if narrow:
        raise XnwanError('narrow tiles are not served by the tiled stepper family')
    if x_cot_ones and not (want_x and want_params):
        raise XnwanError('x_cot_ones needs want_x and want_params')
    if not (want_x or want_params):
        raise XnwanError('a sweep produces x outputs, parameter gradients or both')
    L, d, P = _launch_dims(jobs, t, theta, H, K)
    arr = (XwOdeBwdJob * len(jobs))()
    for a, j in zip(arr, jobs):
        _sweep_job(a, j, d, L, H, P, want_x, want_params, x_cot_ones, lib.xw_tiled_ode_bwd_slabs)
    mode = _mode_word(want_x, want_params, x_cot_ones, prio_drop=prio_drop)
    work = tiled_ode_work(True, d, H, K, m, sum(lib.xw_tiled_ode_bwd_slabs(a.N) for a in arr), t.device, method)
    entry, sel = ('xw_adams_tiled_bwd_multi', ()) if method == ADAMS else ('xw_tiled_ode_bwd_multi', (method,))
    check(getattr(lib, entry)(arr, len(jobs), _p(t), _p(theta), *sel, L, d, H, K, m, mode, _p(work), _stream()), entry)


def tiled_ode_fwd(xT, t, start, theta, method, H, K, m, want_Y=True):
    """u_theta on N paths on the tiled family: (u[L,N], Y[L,H,N] or None)"""
    d, N = xT.shape
    L = t.shape[0]
    u = torch.empty(L, N, dtype=F64, device=xT.device)
    Y = torch.empty(L, H, N, dtype=F64, device=xT.device) if want_Y else None
    tiled_ode_fwd_multi([dict(xT=xT, start=start, u=u, Y=Y)], t, theta, method, H, K, m)
    return u, Y


def tiled_paths_fwd(jobs, theta, method, H, K, m, last_only=False):
    """the tiled family's forward pass over ragged groups (csrc/xw_tiled_paths.hip): job = dict(xT[d,N], start[N], tT[L,N] -- a
    non-decreasing time grid per path, a shorter path repeating its last time --, u[L,N] (last_only: [N]), optional Y[L,H,N]
    (last_only: [H,N]) and nstep[N] int32, the index of each path's last distinct time); theta at the widths (H, K), the generic
    layout.  One L for all jobs of a launch."""
    _need_gpu()
    d = jobs[0]['xT'].shape[0]
    L = jobs[0]['tT'].shape[0]
    _chk(theta, F64, (theta_size(d, H, K),), 'theta')
    if method not in METHODS.values():
        raise XnwanError('per-path time grids run the fixed-grid methods %s only (no per-path step controller or history is built)'
                         % sorted(METHODS))
    arr = (XwPathsJob * len(jobs))()
    for a, j in zip(arr, jobs):
        N = j['xT'].shape[1]
        _chk(j['xT'], F64, (d, N), 'xT'); _chk(j['start'], F64, (N,), 'start'); _chk(j['tT'], F64, (L, N), 'tT')
        _chk(j.get('nstep'), torch.int32, (N,), 'nstep')
        _chk(j['u'], F64, (N,) if last_only else (L, N), 'u'); _chk(j.get('Y'), F64, (H, N) if last_only else (L, H, N), 'Y')
        a.xT, a.start, a.tT, a.nstep, a.u, a.Y = _p(j['xT']), _p(j['start']), _p(j['tT']), _p(j.get('nstep')), _p(j['u']), _p(j.get('Y'))
        a.N, a.last_only = N, 1 if last_only else 0
    # (xw_paths_tiled_work is the forward workspace of the family, xw_tiled_ode_work(0, ...): one allocation helper for both)
    work = tiled_ode_work(False, d, H, K, m, sum(lib.xw_tiled_ode_bwd_slabs(a.N) for a in arr), theta.device)
    check(lib.xw_paths_tiled_fwd(arr, len(jobs), _p(theta), method, L, d, H, K, m, _p(work), _stream()), 'xw_paths_tiled_fwd')


def tiled_paths_grad(jobs, theta, method, H, K, m):
    """the reverse sweep behind tiled_paths_fwd (csrc/xw_tiled_paths_grad.hip, include/xnwan_grad.h): job = dict(xT[d,N], start[N],
    tT[L,N], optional nstep[N] int32 -- as the forward pass took them --, Y[L,H,N], the checkpoints that forward pass wrote (not
    last_only), and the outputs asked for, at least one of gx[d,N], gs[N], ut[N]).  With the cotangent 1 on every path's final value
    u_p: gx = du_p/dx_p and gs = du_p/dstart_p, the discrete adjoint (the exact reverse of the steps taken, grid and step sizes held
    fixed); ut = FL_w . F(t_p, x_p, y(t_p)), the time derivative of the CONTINUOUS model at fixed x -- not the derivative of the
    discrete u with respect to the end of its grid.  One L for all jobs of a launch."""
    _need_gpu()
    d = jobs[0]['xT'].shape[0]
    L = jobs[0]['tT'].shape[0]
    _chk(theta, F64, (theta_size(d, H, K),), 'theta')
    if method not in METHODS.values():
        raise XnwanError('per-path time grids run the fixed-grid methods %s only (no per-path step controller or history is built)'
                         % sorted(METHODS))
    arr = (XwPathsGradJob * len(jobs))()
    for a, j in zip(arr, jobs):
        N = j['xT'].shape[1]
        _chk(j['xT'], F64, (d, N), 'xT'); _chk(j['start'], F64, (N,), 'start'); _chk(j['tT'], F64, (L, N), 'tT')
        _chk(j.get('nstep'), torch.int32, (N,), 'nstep')
        if j.get('Y') is None:
            raise XnwanError('tiled_paths_grad: Y [L, H, N], the checkpoints of tiled_paths_fwd, is needed (the forward is not recomputed)')
        _chk(j['Y'], F64, (L, H, N), 'Y')
        if j.get('gx') is None and j.get('gs') is None and j.get('ut') is None:
            raise XnwanError('tiled_paths_grad: no output requested (at least one of gx, gs, ut)')
        _chk(j.get('gx'), F64, (d, N), 'gx'); _chk(j.get('gs'), F64, (N,), 'gs'); _chk(j.get('ut'), F64, (N,), 'ut')
        a.xT, a.start, a.tT, a.nstep, a.Y = _p(j['xT']), _p(j['start']), _p(j['tT']), _p(j.get('nstep')), _p(j['Y'])
        a.gx, a.gs, a.ut, a.N = _p(j.get('gx')), _p(j.get('gs')), _p(j.get('ut')), N
    # (xw_paths_tiled_grad_work is the sweep workspace of the family, xw_tiled_ode_work(1, ...): one allocation helper for both)
    work = tiled_ode_work(True, d, H, K, m, sum(lib.xw_tiled_ode_bwd_slabs(a.N) for a in arr), theta.device)
    check(lib.xw_paths_tiled_grad(arr, len(jobs), _p(theta), method, L, d, H, K, m, _p(work), _stream()), 'xw_paths_tiled_grad')


def paths_hvp_work(d, H, K, m, tiles, device):
    """the workspace of one tiled_paths_hvp launch over `tiles` 16-path tiles (xw_paths_tiled_hvp_work doubles per tile: the
    entry's own size, the gradient sweep's vectors and their tangents)"""
    per = lib.xw_paths_tiled_hvp_work(d, H, K, m)
    check(min(per, 0), 'xw_paths_tiled_hvp_work')
    return torch.empty(per * tiles, dtype=F64, device=device)


def tiled_paths_hvp(jobs, theta, method, H, K, m, work=None):
    """Hessian-vector products behind tiled_paths_fwd (csrc/xw_tiled_paths_hvp.hip, include/xnwan_hess.h): job = dict(xT[d,N],
    start[N], tT[L,N], optional nstep[N] int32, Y[L,H,N] -- as tiled_paths_grad takes them --, the direction vx[d,N] and vs[N], the
    tangent checkpoints Yd[L,H,N] (scratch of the job that the caller allocates; every element is written: row l is the derivative of
    y_l along the direction) and the outputs asked for, at least one of ju[N], hx[d,N], hs[N]).  With U_p(x, s) the DISCRETE final
    value of path p, grid and step sizes held fixed: ju = dU_p/dx . vx_p + dU_p/ds vs_p, and (hx, hs) = the Hessian of U_p in (x, s)
    applied to (vx_p, vs_p) -- the derivative of tiled_paths_grad's (gx, gs) along the direction, ReLU gates constants as autograd
    takes them.  Time is not perturbed.  work: the launch's workspace (paths_hvp_work over the jobs' tiles) when the caller brings
    its own.  One L for all jobs of a launch."""
    _need_gpu()
    d = jobs[0]['xT'].shape[0]
    L = jobs[0]['tT'].shape[0]
    _chk(theta, F64, (theta_size(d, H, K),), 'theta')
    if method not in METHODS.values():
        raise XnwanError('per-path time grids run the fixed-grid methods %s only (no per-path step controller or history is built)'
                         % sorted(METHODS))
    arr = (XwPathsHvpJob * len(jobs))()
    for a, j in zip(arr, jobs):
        N = j['xT'].shape[1]
        _chk(j['xT'], F64, (d, N), 'xT'); _chk(j['start'], F64, (N,), 'start'); _chk(j['tT'], F64, (L, N), 'tT')
        _chk(j.get('nstep'), torch.int32, (N,), 'nstep')
        if j.get('Y') is None:
            raise XnwanError('tiled_paths_hvp: Y [L, H, N], the checkpoints of tiled_paths_fwd, is needed (the forward is not recomputed)')
        _chk(j['Y'], F64, (L, H, N), 'Y')
        for k in ('vx', 'vs', 'Yd'):
            if j.get(k) is None:
                raise XnwanError('tiled_paths_hvp: %s is needed (the direction vx [d, N] and vs [N]; Yd [L, H, N], the tangent '
                                 'checkpoints the launch writes)' % k)
        _chk(j['vx'], F64, (d, N), 'vx'); _chk(j['vs'], F64, (N,), 'vs'); _chk(j['Yd'], F64, (L, H, N), 'Yd')
        if j.get('ju') is None and j.get('hx') is None and j.get('hs') is None:
            raise XnwanError('tiled_paths_hvp: no output requested (at least one of ju, hx, hs)')
        _chk(j.get('ju'), F64, (N,), 'ju'); _chk(j.get('hx'), F64, (d, N), 'hx'); _chk(j.get('hs'), F64, (N,), 'hs')
        a.xT, a.start, a.tT, a.nstep, a.Y = _p(j['xT']), _p(j['start']), _p(j['tT']), _p(j.get('nstep')), _p(j['Y'])
        a.vx, a.vs, a.Yd, a.ju, a.hx, a.hs, a.N = _p(j['vx']), _p(j['vs']), _p(j['Yd']), _p(j.get('ju')), _p(j.get('hx')), _p(j.get('hs')), N
    tiles = sum((a.N + 15) // 16 for a in arr)
    if work is None:
        work = paths_hvp_work(d, H, K, m, tiles, theta.device)
    else:
        _chk(work, F64, (lib.xw_paths_tiled_hvp_work(d, H, K, m) * tiles,), 'work')
    check(lib.xw_paths_tiled_hvp(arr, len(jobs), _p(theta), method, L, d, H, K, m, _p(work), _stream()), 'xw_paths_tiled_hvp')


def paths_jet_work(d, H, K, m, blocks, device):
    """the workspace of one tiled_paths_jet launch over `blocks` blocks, the jobs' sum of R * ((N + 15) // 16)
    (xw_paths_tiled_jet_work doubles per block: the sweep's vectors, which keep every layer's gates, and the second order's)"""
    per = lib.xw_paths_tiled_jet_work(d, H, K, m)
    check(min(per, 0), 'xw_paths_tiled_jet_work')
    return torch.empty(per * blocks, dtype=F64, device=device)


def tiled_paths_jet(jobs, theta, method, H, K, m, work=None):
    """second-order forward jets behind tiled_paths_fwd's inputs (csrc/xw_tiled_paths_jet.hip, include/xnwan_jet.h): job =
    dict(xT[d,N], start[N], tT[L,N], optional nstep[N] int32 -- as tiled_paths_fwd takes them; NO checkpoints --, R curves per path
    vx[R,d,N], vs[R,N] and optional qs[R,N] (None: zeros), and the outputs asked for: optional u[N], at least one of ju[R,N],
    quu[R,N]).  With U_p(x, s) the DISCRETE final value of path p, grid and step sizes held fixed, along
    gamma(eps) = (x + eps vx, s + eps vs + eps^2 / 2 qs): ju = d/deps U(gamma) = dU/dx . vx + dU/ds vs and quu = d^2/deps^2
    U(gamma) = (vx, vs)^T Hess U (vx, vs) + dU/ds qs at eps = 0, ReLU gates constants as autograd takes them; u = U_p, the bits of
    tiled_paths_fwd.  Time is not perturbed.  work: the launch's workspace (paths_jet_work over the jobs' blocks) when the caller
    brings its own.  One L for all jobs of a launch."""
    _need_gpu()
    d = jobs[0]['xT'].shape[0]
    L = jobs[0]['tT'].shape[0]
    _chk(theta, F64, (theta_size(d, H, K),), 'theta')
    if method not in METHODS.values():
        raise XnwanError('per-path time grids run the fixed-grid methods %s only (no per-path step controller or history is built)'
                         % sorted(METHODS))
    arr = (XwPathsJetJob * len(jobs))()
    for a, j in zip(arr, jobs):
        N = j['xT'].shape[1]
        _chk(j['xT'], F64, (d, N), 'xT'); _chk(j['start'], F64, (N,), 'start'); _chk(j['tT'], F64, (L, N), 'tT')
        _chk(j.get('nstep'), torch.int32, (N,), 'nstep')
        for k in ('vx', 'vs'):
            if j.get(k) is None:
                raise XnwanError('tiled_paths_jet: %s is needed (the directions vx [R, d, N] and vs [R, N])' % k)
        if not (torch.is_tensor(j['vx']) and j['vx'].dim() == 3 and j['vx'].shape[0] >= 1):
            raise XnwanError('tiled_paths_jet: vx must be a tensor [R, d, N] with R >= 1 directions per path')
        R = j['vx'].shape[0]
        _chk(j['vx'], F64, (R, d, N), 'vx'); _chk(j['vs'], F64, (R, N), 'vs'); _chk(j.get('qs'), F64, (R, N), 'qs')
        if j.get('ju') is None and j.get('quu') is None:
            raise XnwanError('tiled_paths_jet: no output requested (at least one of ju, quu)')
        _chk(j.get('u'), F64, (N,), 'u'); _chk(j.get('ju'), F64, (R, N), 'ju'); _chk(j.get('quu'), F64, (R, N), 'quu')
        a.xT, a.start, a.tT, a.nstep = _p(j['xT']), _p(j['start']), _p(j['tT']), _p(j.get('nstep'))
        a.vx, a.vs, a.qs, a.N, a.R = _p(j['vx']), _p(j['vs']), _p(j.get('qs')), N, R
        a.u, a.ju, a.quu = _p(j.get('u')), _p(j.get('ju')), _p(j.get('quu'))
    blocks = sum(a.R * ((a.N + 15) // 16) for a in arr)
    if work is None:
        work = paths_jet_work(d, H, K, m, blocks, theta.device)
    else:
        _chk(work, F64, (lib.xw_paths_tiled_jet_work(d, H, K, m) * blocks,), 'work')
    check(lib.xw_paths_tiled_jet(arr, len(jobs), _p(theta), method, L, d, H, K, m, _p(work), _stream()), 'xw_paths_tiled_jet')


def paths_vjp_work(d, H, K, m, tiles, device):
    """the workspace of one tiled_paths_vjp launch over `tiles` 16-path tiles (xw_paths_tiled_vjp_work doubles per tile: the
    gradient sweep's vectors and the 16 stage times of the tile's paths)"""
    per = lib.xw_paths_tiled_vjp_work(d, H, K, m)
    check(min(per, 0), 'xw_paths_tiled_vjp_work')
    return torch.empty(per * tiles, dtype=F64, device=device)


def tiled_paths_vjp(jobs, theta, method, H, K, m, work=None):
    """parameter gradients behind tiled_paths_fwd (csrc/xw_tiled_paths_vjp.hip, include/xnwan_vjp.h): job = dict(xT[d,N], start[N],
    tT[L,N], optional nstep[N] int32, Y[L,H,N] -- as tiled_paths_grad takes them --, a weight per path w[N], the slabs
    gslab[xw_tiled_ode_bwd_slabs(N), P_u] (P_u = theta's size; zeroed by the launch, every element written) and optional gx[d,N],
    gs[N]).  With U_p(theta) the DISCRETE final value of path p -- the exact reverse of the steps taken, the grid and the step sizes
    held fixed, the start value a constant of theta, ReLU gates constants as autograd takes them --: slab_sum(gslab) = sum_p w_p
    dU_p/dtheta in theta's layout, gx = w_p dU_p/dx_p, gs = w_p dU_p/dstart_p.  A path with w_p = 0 adds exact zeros.  work: the
    launch's workspace (paths_vjp_work over the jobs' tiles) when the caller brings its own.  One L for all jobs of a launch."""
    _need_gpu()
    d = jobs[0]['xT'].shape[0]
    L = jobs[0]['tT'].shape[0]
    P = theta_size(d, H, K)
    _chk(theta, F64, (P,), 'theta')
    if method not in METHODS.values():
        raise XnwanError('per-path time grids run the fixed-grid methods %s only (no per-path step controller or history is built)'
                         % sorted(METHODS))
    arr = (XwPathsVjpJob * len(jobs))()
    for a, j in zip(arr, jobs):
        N = j['xT'].shape[1]
        _chk(j['xT'], F64, (d, N), 'xT'); _chk(j['start'], F64, (N,), 'start'); _chk(j['tT'], F64, (L, N), 'tT')
        _chk(j.get('nstep'), torch.int32, (N,), 'nstep')
        if j.get('Y') is None:
            raise XnwanError('tiled_paths_vjp: Y [L, H, N], the checkpoints of tiled_paths_fwd, is needed (the forward is not recomputed)')
        _chk(j['Y'], F64, (L, H, N), 'Y')
        for k in ('w', 'gslab'):
            if j.get(k) is None:
                raise XnwanError('tiled_paths_vjp: %s is needed (the weights w [N]; gslab [(N + 15) // 16, P_u], the slabs the '
                                 'launch writes)' % k)
        _chk(j['w'], F64, (N,), 'w'); _chk(j['gslab'], F64, (lib.xw_tiled_ode_bwd_slabs(N), P), 'gslab')
        _chk(j.get('gx'), F64, (d, N), 'gx'); _chk(j.get('gs'), F64, (N,), 'gs')
        a.xT, a.start, a.tT, a.nstep, a.Y = _p(j['xT']), _p(j['start']), _p(j['tT']), _p(j.get('nstep')), _p(j['Y'])
        a.w, a.gslab, a.gx, a.gs, a.N = _p(j['w']), _p(j['gslab']), _p(j.get('gx')), _p(j.get('gs')), N
    tiles = sum((a.N + 15) // 16 for a in arr)
    if work is None:
        work = paths_vjp_work(d, H, K, m, tiles, theta.device)
    else:
        _chk(work, F64, (lib.xw_paths_tiled_vjp_work(d, H, K, m) * tiles,), 'work')
    check(lib.xw_paths_tiled_vjp(arr, len(jobs), _p(theta), method, L, d, H, K, m, _p(work), _stream()), 'xw_paths_tiled_vjp')


def paths_gvjp_work(d, H, K, m, tiles, device):
    """the workspace of one tiled_paths_gvjp launch over `tiles` 16-path tiles (xw_paths_tiled_gvjp_work doubles per tile: the
    Hessian-vector sweep's vectors, the stage times and weights of the tile's paths and a tangent per layer of the field)"""
    per = lib.xw_paths_tiled_gvjp_work(d, H, K, m)
    check(min(per, 0), 'xw_paths_tiled_gvjp_work')
    return torch.empty(per * tiles, dtype=F64, device=device)


def tiled_paths_gvjp(jobs, theta, method, H, K, m, work=None):
    """parameter gradients of u, of its derivative along a direction and of ut behind tiled_paths_fwd (csrc/xw_tiled_paths_gvjp.hip,
    include/xnwan_grad_vjp.h): job = dict(xT[d,N], start[N], tT[L,N], optional nstep[N] int32, Y[L,H,N] -- as tiled_paths_grad takes
    them --, the slabs gslab[xw_tiled_ode_bwd_slabs(N), P_u] (P_u = theta's size; zeroed by the launch, every element written) and at
    least one of: wu[N], a weight on u; wt[N], a weight on ut; the direction vx[d,N] with vs[N] and Yd[L,H,N], the tangent
    checkpoints that tiled_paths_hvp wrote for this direction (run it with ju alone first: Yd is READ here)).  With U_p(theta; x, s)
    the DISCRETE final value of path p -- the exact reverse of the steps taken, the grid and the step sizes held fixed, the start
    value and the direction constants of theta, ReLU gates constants as autograd takes them -- and ut_p = FL_w . F(t_p, x_p, y(t_p)):
    slab_sum(gslab) = d/dtheta sum_p [wu_p U_p + (dU_p/dx . vx_p + dU_p/ds vs_p) + wt_p ut_p] in theta's layout.  A path whose
    weights and direction are zero adds exact zeros.  work: the launch's workspace (paths_gvjp_work over the jobs' tiles) when the
    caller brings its own.  One L for all jobs of a launch."""
    _need_gpu()
    d = jobs[0]['xT'].shape[0]
    L = jobs[0]['tT'].shape[0]
    P = theta_size(d, H, K)
    _chk(theta, F64, (P,), 'theta')
    if method not in METHODS.values():
        raise XnwanError('per-path time grids run the fixed-grid methods %s only (no per-path step controller or history is built)'
                         % sorted(METHODS))
    arr = (XwPathsGvjpJob * len(jobs))()
    for a, j in zip(arr, jobs):
        N = j['xT'].shape[1]
        _chk(j['xT'], F64, (d, N), 'xT'); _chk(j['start'], F64, (N,), 'start'); _chk(j['tT'], F64, (L, N), 'tT')
        _chk(j.get('nstep'), torch.int32, (N,), 'nstep')
        if j.get('Y') is None:
            raise XnwanError('tiled_paths_gvjp: Y [L, H, N], the checkpoints of tiled_paths_fwd, is needed (the forward is not recomputed)')
        _chk(j['Y'], F64, (L, H, N), 'Y')
        if j.get('gslab') is None:
            raise XnwanError('tiled_paths_gvjp: gslab [(N + 15) // 16, P_u], the slabs the launch writes, is needed')
        _chk(j['gslab'], F64, (lib.xw_tiled_ode_bwd_slabs(N), P), 'gslab')
        direction = j.get('vx') is not None
        if direction != (j.get('vs') is not None):
            raise XnwanError('tiled_paths_gvjp: vx [d, N] and vs [N] are one direction: both or neither')
        if direction and j.get('Yd') is None:
            raise XnwanError('tiled_paths_gvjp: Yd [L, H, N], the tangent checkpoints tiled_paths_hvp wrote for (vx, vs), is needed '
                             'with a direction (the tangent forward is not recomputed)')
        if not direction and j.get('wu') is None and j.get('wt') is None:
            raise XnwanError('tiled_paths_gvjp: nothing to differentiate (at least one of wu, wt, vx with vs)')
        _chk(j.get('vx'), F64, (d, N), 'vx'); _chk(j.get('vs'), F64, (N,), 'vs')
        _chk(j.get('Yd') if direction else None, F64, (L, H, N), 'Yd')
        _chk(j.get('wu'), F64, (N,), 'wu'); _chk(j.get('wt'), F64, (N,), 'wt')
        a.xT, a.start, a.tT, a.nstep, a.Y = _p(j['xT']), _p(j['start']), _p(j['tT']), _p(j.get('nstep')), _p(j['Y'])
        a.Yd, a.vx, a.vs = _p(j.get('Yd') if direction else None), _p(j.get('vx')), _p(j.get('vs'))
        a.wu, a.wt, a.gslab, a.N = _p(j.get('wu')), _p(j.get('wt')), _p(j['gslab']), N
    tiles = sum((a.N + 15) // 16 for a in arr)
    if work is None:
        work = paths_gvjp_work(d, H, K, m, tiles, theta.device)
    else:
        _chk(work, F64, (lib.xw_paths_tiled_gvjp_work(d, H, K, m) * tiles,), 'work')
    check(lib.xw_paths_tiled_gvjp(arr, len(jobs), _p(theta), method, L, d, H, K, m, _p(work), _stream()), 'xw_paths_tiled_gvjp')


def tiled_ode_bwd(xT, t, start, theta, Y, ubar, method, H, K, m, want_x=True, want_params=False):
    """the reverse sweep on the tiled family: (gx[d,N], gs[N], gslab[nslab,P_u]) -- entries not requested are None"""
    d, N = xT.shape
    dev = xT.device
    gx = torch.empty(d, N, dtype=F64, device=dev) if want_x else None
    gs = torch.empty(N, dtype=F64, device=dev) if want_x else None
    gslab = torch.empty(lib.xw_tiled_ode_bwd_slabs(N), theta_size(d, H, K), dtype=F64, device=dev) if want_params else None
    tiled_ode_bwd_multi([dict(xT=xT, start=start, Y=Y, ubar=ubar, gx=gx, gs=gs, gslab=gslab)], t, theta, method, H, K, m,
                        want_x, want_params)
    return gx, gs, gslab


def ode_bwd_slabs(N):
    return lib.xw_ode_bwd_slabs(N)


def ode_act_cols(N):
    """columns of the activation store for N paths: whole tiles of 16 (the store is tile-major inside a step)"""
    return (N + 15) // 16 * 16


def ode_act_rows(method, H, K, m):
    """rows per step of the activation store that ode_fwd_multi fills and ode_bwd_multi reads (0: not used by `method`)"""
    r = lib.xw_ode_act_rows(int(method), H, K, m)
    check(min(r, 0), 'xw_ode_act_rows')
    return r


def ode_bwd(xT, t, start, theta, Y, ubar, method, H, K, m, want_x=True, want_params=False, gx=None, gs=None, gslab=None,
            adjoint=False):
    """reverse sweep: returns (gx[d,N], gs[N], gslab[nslab,P_u]) -- entries not requested are None."""
    _need_gpu()
    d, N = xT.shape
    L = t.shape[0]
    P = theta_size(d, H, K)
    _chk(xT, F64, (d, N), 'xT'); _chk(t, F64, (L,), 't'); _chk(start, F64, (N,), 'start'); _chk(theta, F64, (P,), 'theta')
    _chk(Y, F64, (L, H, N), 'Y'); _chk(ubar, F64, (L, N), 'ubar')
    mode = _mode_word(want_x, want_params, adjoint=adjoint)
    if want_x:
        gx = torch.empty(d, N, dtype=F64, device=xT.device) if gx is None else gx
        gs = torch.empty(N, dtype=F64, device=xT.device) if gs is None else gs
        _chk(gx, F64, (d, N), 'gx'); _chk(gs, F64, (N,), 'gs')
    if want_params:
        ns = ode_bwd_slabs(N)
        gslab = torch.empty(ns, P, dtype=F64, device=xT.device) if gslab is None else gslab
        _chk(gslab, F64, (ns, P), 'gslab')
    check(lib.xw_ode_bwd(_p(xT), _p(t), _p(start), _p(theta), _p(Y), _p(ubar), method, N, L, d, H, K, m, mode,
                         _p(gx if want_x else None), _p(gs if want_x else None), _p(gslab if want_params else None),
                         _stream()), 'xw_ode_bwd')
    return (gx if want_x else None), (gs if want_x else None), (gslab if want_params else None)


def family_ode_fwd(xT, t, start, theta, method, H, K, m, want_Y=True, family=None):
    """ode_fwd or tiled_ode_fwd (neither routes to the other) for one group and a fixed-grid method, by the family that runs
    (H, K, m): `family`, or stepper_family's under the default policy"""
    if (family or stepper_family(H, K, m, method=method)) == 'tiled':       # (H, K: theta's widths -- the network's own on this family)
        return tiled_ode_fwd(xT, t, start, theta, method, H, K, m, want_Y=want_Y)
    return ode_fwd(xT, t, start, theta, method, H, K, m, want_Y=want_Y)


def family_ode_bwd(xT, t, start, theta, Y, ubar, method, H, K, m, want_x=True, want_params=False, adjoint=False, family=None):
    """ode_bwd / tiled_ode_bwd for one group, chosen as in family_ode_fwd: (gx, gs, gslab)"""
    if (family or stepper_family(H, K, m, method=method)) != 'tiled':
        return ode_bwd(xT, t, start, theta, Y, ubar, method, H, K, m, want_x=want_x, want_params=want_params, adjoint=adjoint)
    if adjoint:
        raise _tiled_adjoint_refused(H, K, m)
    return tiled_ode_bwd(xT, t, start, theta, Y, ubar, method, H, K, m, want_x=want_x, want_params=want_params)


# ----------------------------------------------------------------------------------------------------------------------
# solver 'dopri5' (csrc/xw_dopri.hip, include/xnwan.h): torchdiffeq's adaptive Dormand-Prince 5(4), one step size per job
# ----------------------------------------------------------------------------------------------------------------------
DOPRI5_RTOL, DOPRI5_ATOL = 1e-7, 1e-9      # torchdiffeq's defaults (the reference passes neither)
DOPRI5_CHUNK, DOPRI5_MAX_STEPS = 8, 10000  # attempts per host check; accepted steps per call (defaults of EngineOptions.dopri5_*)
DOPRI5_MAXJOBS = 8                         # jobs per launch (csrc/xw_dopri_ctl.h XW_DOPRI_MAXJOBS)
DOPRI5_STEPPERS = ('vector', 'tiled')      # the two implementations: csrc/xw_dopri.hip (the field per path on the vector ALU, up to
                                           # GENERIC_ODE_MAX) and csrc/xw_tdopri.hip (per 16-path tile on the MFMA, up to TILED_ODE_MAX)
# per stepper: the init, attempts and sweep entry points, the size of a record's partial sums (per 64-path block, or per 16-path
# tile), and whether the launches take a workspace (_dopri5_tiled_work) ahead of the stream
_DOPRI5_ENTRY = {'vector': ('xw_dopri5_init', 'xw_dopri5_attempts', 'xw_dopri5_sweep', 'xw_dopri5_work_size', False),
                 'tiled': ('xw_tdopri5_init', 'xw_tdopri5_attempts', 'xw_tdopri5_sweep', 'xw_tdopri5_part_size', True)}
CTL_T0, CTL_DT, CTL_NACC, CTL_NATT, CTL_DONE, CTL_STATUS, CTL_RATIO, CTL_GAP = 0, 1, 2, 3, 4, 5, 8, 9


def dopri5_stepper(name):
    """`name` if it is one of DOPRI5_STEPPERS (EngineOptions.dopri5_stepper, XNODE.dopri5_stepper), else XnwanError"""
    if name not in DOPRI5_STEPPERS:
        raise XnwanError("dopri5_stepper = %r: one of 'vector' (csrc/xw_dopri.hip, the field on the vector ALU, widths up to %s) "
                         "and 'tiled' (csrc/xw_tdopri.hip, the field on the tiled MFMA stepper, widths up to %s)"
                         % (name, GENERIC_ODE_MAX, TILED_ODE_MAX))
    return name


def _dopri5_tiled_work(sweep, d, H, K, m, Ns, dev):
    """the per-launch workspace of the tiled dopri5 kernels for jobs of Ns paths (xw_tdopri5_work doubles per 16-path tile)"""
    per = lib.xw_tdopri5_work(1 if sweep else 0, d, H, K, m)
    check(min(per, 0), 'xw_tdopri5_work')
    return torch.empty(per * sum((N + 15) // 16 for N in Ns), dtype=F64, device=dev)


def dopri5_status_message(status, ctl, max_steps):
    """the XnwanError text for a controller that ended with `status` (include/xnwan.h XW_DOPRI_*); None for status 0.
    ctl: the job's controller as a host sequence (t0, dt, ... slots)"""
    status = int(status)
    if status == 0:
        return None
    where = 'at t = %.17g after %d accepted steps / %d attempts' % (float(ctl[CTL_T0]), int(ctl[CTL_NACC]), int(ctl[CTL_NATT]))
    if status == 1:
        return "solver 'dopri5': underflow in dt %.17g %s (t0 + dt == t0)" % (float(ctl[CTL_DT]), where)
    if status == 2:
        return ("solver 'dopri5': the step limit of %d accepted steps (EngineOptions.dopri5_max_steps / XNODE.dopri5_max_steps) "
                "was reached before the last sample time, %s" % (int(max_steps), where))
    if status == 3:
        return "solver 'dopri5': the error ratio is not finite (NaN in the field?) %s" % where
    if status == 4:
        return "solver 'dopri5': the step record is full %s -- the host did not grow it ahead of the attempts" % where
    return "solver 'dopri5': unknown controller status %d %s" % (status, where)


class Dopri5Record:
    """What a dopri5 forward pass leaves for its sweep: per job the states at the accepted grid points, the grid, the step
    sizes and the controller.  `n_acc`, `n_att`, `min_gap`, `grid` (host float64 tensor) and `steps` (accepted (t0, dt)) are
    filled when dopri5_fwd returns."""

    def __init__(self, N, H, cap, dev, stepper='vector'):
        self.N, self.H, self.cap, self.stepper = N, H, cap, dopri5_stepper(stepper)
        self.rec_y = torch.empty(cap + 1, H, N, dtype=F64, device=dev)
        self.rec_t = torch.empty(cap + 1, dtype=F64, device=dev)
        self.rec_h = torch.empty(max(cap, 1), dtype=F64, device=dev)
        self.fbuf = torch.empty(2, H, N, dtype=F64, device=dev)
        # (the partial sums of the forward's reductions -- the sweeps do not read them)
        self.work = torch.empty(getattr(lib, _DOPRI5_ENTRY[stepper][3])(N), dtype=F64, device=dev)
        self.n_acc = self.n_att = 0
        self.grid = self.min_gap = self.steps = None

    def grow(self, cap, n_acc):
        """a larger record holding the first n_acc + 1 grid points of this one (stream-ordered copies)"""
        y, tt, h = self.rec_y, self.rec_t, self.rec_h
        self.rec_y = torch.empty(cap + 1, self.H, self.N, dtype=F64, device=y.device)
        self.rec_t = torch.empty(cap + 1, dtype=F64, device=y.device)
        self.rec_h = torch.empty(cap, dtype=F64, device=y.device)
        self.rec_y[:n_acc + 1].copy_(y[:n_acc + 1])
        self.rec_t[:n_acc + 1].copy_(tt[:n_acc + 1])
        self.rec_h[:n_acc].copy_(h[:n_acc])
        self.cap = cap


def dopri5_fwd(jobs, t, theta, H, K, m, Hn, rtol=DOPRI5_RTOL, atol=DOPRI5_ATOL, chunk=DOPRI5_CHUNK, max_steps=DOPRI5_MAX_STEPS,
               cap=None, stepper='vector'):
    """u_theta with solver 'dopri5' for jobs = list of dicts(xT[d,N], start[N], u[L,N], Y[L,H,N] or None) sharing t and theta;
    one step size per job (one odeint call of the reference).  Hn: the network's u_hidden_dim (the RMS norms divide by N Hn).
    Enqueues the init launches, then attempts in chunks of `chunk` launches; after each chunk the controllers are copied to
    page-locked host memory and ONE event is waited on; the records grow on the host before the next chunk, so that no attempt
    can write past them.  Returns a Dopri5Record per job (for dopri5_sweep and diagnostics).  A controller that ends with a bad
    status raises XnwanError.  Synchronises with the host: a dopri5 forward cannot be captured into a graph.
    stepper: 'vector' (xw_dopri5_*) or 'tiled' (xw_tdopri5_*: H, K up to 256, m up to 32; one workspace for all its launches)."""
    _need_gpu()
    init, attempts, _, _, takes_work = _DOPRI5_ENTRY[dopri5_stepper(stepper)]
    if not 1 <= len(jobs) <= DOPRI5_MAXJOBS:
        raise XnwanError('dopri5_fwd: 1 .. %d jobs per call, got %d' % (DOPRI5_MAXJOBS, len(jobs)))
    chunk, max_steps = int(chunk), int(max_steps)
    if chunk < 1 or max_steps < 1:
        raise XnwanError('dopri5_fwd: chunk and max_steps must be >= 1')
    L, d, _ = _launch_dims(jobs, t, theta, H, K)
    nj, dev = len(jobs), t.device
    ctl = torch.zeros(nj, lib.xw_dopri5_ctl_size(), dtype=F64, device=dev)
    mirror = torch.empty(ctl.shape, dtype=F64, pin_memory=True)
    arr = (XwDopriJob * nj)()
    recs = [Dopri5Record(_fwd_job(a, j, d, L, H, hints=False), H, int(cap) if cap else 4 * chunk, dev, stepper) for a, j in zip(arr, jobs)]
    work = _dopri5_tiled_work(False, d, H, K, m, [r.N for r in recs], dev) if takes_work else None
    tail = (_p(work), _stream()) if takes_work else (_stream(),)

    def fill():                            # (the record's fields: again after a record has grown)
        for i, (a, r) in enumerate(zip(arr, recs)):
            a.rec_y, a.rec_t, a.rec_h, a.fbuf = _p(r.rec_y), _p(r.rec_t), _p(r.rec_h), _p(r.fbuf)
            a.ctl, a.work, a.cap = _p(ctl[i]), _p(r.work), r.cap
    args = (_p(t), _p(theta), L, d, H, K, m, int(Hn), float(rtol), float(atol))
    fill()
    check(getattr(lib, init)(arr, nj, *args, *tail), init)
    ev = torch.cuda.Event()
    n_acc = [0] * nj
    while True:
        grown = False
        for i, r in enumerate(recs):
            if r.cap < n_acc[i] + chunk:
                r.grow(max(2 * r.cap, n_acc[i] + chunk), n_acc[i])
                grown = True
        if grown:
            fill()
        check(getattr(lib, attempts)(arr, nj, *args, max_steps, chunk, *tail), attempts)
        mirror.copy_(ctl, non_blocking=True)
        ev.record()
        ev.synchronize()
        n_acc = [int(c) for c in mirror[:, CTL_NACC].tolist()]
        if all(mirror[:, CTL_DONE] != 0):
            break
    host = mirror.clone()
    for i, r in enumerate(recs):
        msg = dopri5_status_message(host[i, CTL_STATUS], host[i], max_steps)
        if msg is not None:
            raise XnwanError(msg)
        r.ctl = ctl[i]
        r.n_acc, r.n_att, r.min_gap = int(host[i, CTL_NACC]), int(host[i, CTL_NATT]), float(host[i, CTL_GAP])
        r.grid = r.rec_t[:r.n_acc + 1].cpu()
        r.steps = list(zip(r.grid[:-1].tolist(), r.rec_h[:r.n_acc].cpu().tolist()))     # accepted (t0, dt)
    return recs


def u_forward(xT, t, start, theta, method, H, K, m, Hn, chunk=DOPRI5_CHUNK, max_steps=DOPRI5_MAX_STEPS, stepper='vector', family=None):
    """u[L,N] of one group with any served solver: family_ode_fwd for the fixed-grid methods, dopri5_fwd (one job) for DOPRI5.
    Hn: the network's u_hidden_dim (dopri5's RMS norms); stepper: dopri5's implementation (DOPRI5_STEPPERS)"""
    if method != DOPRI5:
        return family_ode_fwd(xT, t, start, theta, method, H, K, m, want_Y=False, family=family)[0]
    u = torch.empty(t.shape[0], xT.shape[1], dtype=F64, device=xT.device)
    dopri5_fwd([dict(xT=xT, start=start, u=u)], t, theta, H, K, m, Hn, chunk=chunk, max_steps=max_steps, stepper=stepper)
    return u


def paths_dopri5_fwd(jobs, theta, H, K, m, Hn, rtol=DOPRI5_RTOL, atol=DOPRI5_ATOL, max_steps=DOPRI5_MAX_STEPS, max_attempts=None):
    """solver 'dopri5' with a step controller PER PATH (csrc/xw_tdopri_paths.hip, include/xnwan_eval.h): every path is one odeint
    call of the reference on the one-path group with the sample times [t_in, t_end], the whole integration of a 16-path tile in one
    launch.  job = dict(xT[d,N], start[N], t_in[N], t_end[N] >= t_in, u[N], status[N], n_acc[N], n_att[N] (int32), optional Y[H,N]
    -- the state at t_end --, rec[cap,2,N] -- t0 and dt of each accepted step below cap --, ckpt[cap,H,N] -- the state at the
    start of each accepted step below cap, slot 0 the lifted start value (include/xnwan_eval_grad.h; the same cap as rec's where
    both are given) -- and fin[2,N] -- t0 and dt of every controller when it stopped); theta at the widths (H, K), the generic
    layout; Hn: the network's u_hidden_dim (the RMS norms divide by it).  The same kernel and the same bits with and without ckpt:
    xw_paths_dopri5_ckpt_fwd is called when a job of the launch has one, xw_paths_dopri5_fwd otherwise.
    max_steps: accepted steps per path; max_attempts: rounds of a tile, 2 max_steps unless given -- the kernel's hard bound.  A path that ends at either gets status XW_DOPRI_STEPS (2); nothing is read back here, nothing raised for a status:
    the launch can be captured (the caller reads status, dopri5_status_message words it)."""
    _need_gpu()
    max_steps = int(max_steps)
    max_attempts = 2 * max_steps if max_attempts is None else int(max_attempts)
    if max_steps < 1 or max_attempts < 1:
        raise XnwanError('paths_dopri5_fwd: max_steps and max_attempts must be >= 1')
    d = jobs[0]['xT'].shape[0]
    _chk(theta, F64, (theta_size(d, H, K),), 'theta')
    keep = any(j.get('ckpt') is not None for j in jobs)
    arr = ((XwPathsDopriCkptJob if keep else XwPathsDopriJob) * len(jobs))()
    for a, j in zip(arr, jobs):
        ckpt = j.get('ckpt')
        if keep:
            a.ckpt, a = _p(ckpt), a.f
        N = j['xT'].shape[1]
        _chk(j['xT'], F64, (d, N), 'xT'); _chk(j['start'], F64, (N,), 'start')
        _chk(j['t_in'], F64, (N,), 't_in'); _chk(j['t_end'], F64, (N,), 't_end'); _chk(j['u'], F64, (N,), 'u')
        for k in ('status', 'n_acc', 'n_att'):
            if j.get(k) is None:
                raise XnwanError('paths_dopri5_fwd: a job needs %s[N] (int32)' % k)
            _chk(j[k], torch.int32, (N,), k)
        rec = j.get('rec')
        cap = 0
        if rec is not None:
            if rec.dim() != 3:
                raise XnwanError('rec must have shape (cap, 2, %d), got %s' % (N, tuple(rec.shape)))
            cap = rec.shape[0]
            _chk(rec, F64, (cap, 2, N), 'rec')
        if ckpt is not None:
            if ckpt.dim() != 3 or ckpt.shape[0] < 1 or (rec is not None and ckpt.shape[0] != cap):
                raise XnwanError('ckpt must have shape (cap, %d, %d) with cap >= 1%s, got %s'
                                 % (H, N, '' if rec is None else " = rec's %d" % cap, tuple(ckpt.shape)))
            cap = ckpt.shape[0]
            _chk(ckpt, F64, (cap, H, N), 'ckpt')
        _chk(j.get('Y'), F64, (H, N), 'Y'); _chk(j.get('fin'), F64, (2, N), 'fin')
        a.xT, a.start, a.t_in, a.t_end, a.u = _p(j['xT']), _p(j['start']), _p(j['t_in']), _p(j['t_end']), _p(j['u'])
        a.status, a.n_acc, a.n_att = _p(j['status']), _p(j['n_acc']), _p(j['n_att'])
        a.Y, a.rec, a.fin, a.N, a.cap = _p(j.get('Y')), _p(rec), _p(j.get('fin')), N, cap
    # (xw_paths_dopri5_work is the tiled dopri5 forward's workspace, xw_tdopri5_work(0, ...): one allocation helper for both)
    work = _dopri5_tiled_work(False, d, H, K, m, [j['xT'].shape[1] for j in jobs], theta.device)
    entry = 'xw_paths_dopri5_ckpt_fwd' if keep else 'xw_paths_dopri5_fwd'
    check(getattr(lib, entry)(arr, len(jobs), _p(theta), d, H, K, m, int(Hn), float(rtol), float(atol), max_steps, max_attempts,
                              _p(work), _stream()), entry)


def paths_dopri5_grad(jobs, theta, H, K, m):
    """the reverse sweep behind paths_dopri5_fwd (csrc/xw_tdopri_paths_grad.hip, include/xnwan_eval_grad.h): job = dict(xT[d,N],
    start[N], t_in[N], t_end[N] -- as the forward pass took them --, n_acc[N] int32, rec[cap,2,N] and ckpt[cap,H,N] as that forward
    pass wrote them (every path with status 0 and n_acc <= cap), Y[H,N], its y(t_end), where ut is asked for, and the outputs asked
    for, at least one of gx[d,N], gs[N], ut[N]).  With the cotangent 1 on every path's value u_p: gx = du_p/dx_p and gs =
    du_p/dstart_p, the discrete adjoint (the exact reverse of the accepted steps, the recorded t0 and dt held fixed, the last step
    through its dense output at t_end); ut = FL_w . F(t_end, x_p, Y_p), the time derivative of the CONTINUOUS model at fixed x -- not
    the derivative of the discrete u with respect to the end of its grid.  Slots at or past a path's n_acc are never read.  Nothing
    is read back: the launch can be captured."""
    _need_gpu()
    d = jobs[0]['xT'].shape[0]
    _chk(theta, F64, (theta_size(d, H, K),), 'theta')
    arr = (XwPathsDopriGradJob * len(jobs))()
    for a, j in zip(arr, jobs):
        N = j['xT'].shape[1]
        _chk(j['xT'], F64, (d, N), 'xT'); _chk(j['start'], F64, (N,), 'start')
        _chk(j['t_in'], F64, (N,), 't_in'); _chk(j['t_end'], F64, (N,), 't_end')
        for k in ('n_acc', 'rec', 'ckpt'):
            if j.get(k) is None:
                raise XnwanError('paths_dopri5_grad: %s, as paths_dopri5_fwd wrote it, is needed (the controller is not run again)' % k)
        _chk(j['n_acc'], torch.int32, (N,), 'n_acc')
        rec, ckpt = j['rec'], j['ckpt']
        if rec.dim() != 3 or rec.shape[0] < 1:
            raise XnwanError('rec must have shape (cap, 2, %d) with cap >= 1, got %s' % (N, tuple(rec.shape)))
        cap = rec.shape[0]
        _chk(rec, F64, (cap, 2, N), 'rec'); _chk(ckpt, F64, (cap, H, N), 'ckpt')
        if j.get('gx') is None and j.get('gs') is None and j.get('ut') is None:
            raise XnwanError('paths_dopri5_grad: no output requested (at least one of gx, gs, ut)')
        if j.get('ut') is not None and j.get('Y') is None:
            raise XnwanError('paths_dopri5_grad: ut needs Y [H, N], the forward pass\'s state at t_end')
        _chk(j.get('Y'), F64, (H, N), 'Y')
        _chk(j.get('gx'), F64, (d, N), 'gx'); _chk(j.get('gs'), F64, (N,), 'gs'); _chk(j.get('ut'), F64, (N,), 'ut')
        a.xT, a.start, a.t_in, a.t_end = _p(j['xT']), _p(j['start']), _p(j['t_in']), _p(j['t_end'])
        a.n_acc, a.rec, a.ckpt, a.Y = _p(j['n_acc']), _p(rec), _p(ckpt), _p(j.get('Y'))
        a.gx, a.gs, a.ut, a.N, a.cap = _p(j.get('gx')), _p(j.get('gs')), _p(j.get('ut')), N, cap
    # (xw_paths_dopri5_grad_work is the tiled dopri5 sweep's workspace, xw_tdopri5_work(1, ...): one allocation helper for both)
    work = _dopri5_tiled_work(True, d, H, K, m, [a.N for a in arr], theta.device)
    check(lib.xw_paths_dopri5_grad(arr, len(jobs), _p(theta), d, H, K, m, _p(work), _stream()), 'xw_paths_dopri5_grad')


def dopri5_sweep(jobs, t, theta, H, K, m, want_x, want_params, x_cot_ones=False, stepper='vector'):
    """reverse of the accepted steps of dopri5_fwd (step sizes and grid as constants: DESIGN 8).  jobs: list of dicts as for
    ode_bwd_multi (xT, start, ubar or res, gx, gs, gslab; no Y / act) plus 'rec': the job's Dopri5Record.  Same outputs and
    layouts as ode_bwd_multi (mode bits 0..2).  stepper: 'vector' (xw_dopri5_sweep) or 'tiled' (xw_tdopri5_sweep); either reverses
    a record of either forward at widths both serve."""
    _need_gpu()
    _, _, sweep, _, takes_work = _DOPRI5_ENTRY[dopri5_stepper(stepper)]
    if not 1 <= len(jobs) <= DOPRI5_MAXJOBS:
        raise XnwanError('dopri5_sweep: 1 .. %d jobs per call, got %d' % (DOPRI5_MAXJOBS, len(jobs)))
    if x_cot_ones and not (want_x and want_params):
        raise XnwanError('x_cot_ones needs want_x and want_params')
    L, d, P = _launch_dims(jobs, t, theta, H, K)
    arr = (XwDopriSweepJob * len(jobs))()
    for a, j in zip(arr, jobs):
        N = j['xT'].shape[1]
        r = j['rec']
        if r.N != N or r.H != H:
            raise XnwanError('dopri5_sweep: the record is for N = %d, H = %d' % (r.N, r.H))
        _sweep_job(a.b, j, d, L, H, P, want_x, want_params, x_cot_ones, ode_bwd_slabs, with_Y=False)
        a.rec_y, a.rec_t, a.rec_h, a.ctl = _p(r.rec_y), _p(r.rec_t), _p(r.rec_h), _p(r.ctl)
    mode = _mode_word(want_x, want_params, x_cot_ones)
    work = _dopri5_tiled_work(True, d, H, K, m, [a.b.N for a in arr], t.device) if takes_work else None
    tail = (_p(work), _stream()) if takes_work else (_stream(),)
    check(getattr(lib, sweep)(arr, len(jobs), _p(t), _p(theta), L, d, H, K, m, mode, *tail), sweep)


DISC_UNROLLED_DEPTH = 9   # v_layers of the reference's YAML: the depth the recomputing reverse kernels are compiled for


def disc_recompute(W, q):
    """True when the recomputing reverse kernels (xw_disc_gradx, xw_disc_bwd without a record) exist for this container
    width and depth: the reference's YAML shape only.  Everything else reverses from the record / the fused gradient."""
    return W == 50 and q == DISC_UNROLLED_DEPTH


def disc_act_rows(W, q, family=None):
    """rows of the activation record disc_fwd can store for disc_bwd: the inputs of the q tied layers + tanh(a_q)"""
    if _disc_family(W, q, family) == 'tiled':
        r = lib.xw_disc_tiled_act_rows(W, q)
        check(min(r, 0), 'xw_disc_tiled_act_rows')
        return r
    r = lib.xw_disc_act_rows(W, q)
    check(min(r, 0), 'xw_disc_act_rows')
    return r


def disc_act_view(act, W, q):
    """the record as [tiles of 16 points, (q+1) W rows, 16]: row j W + k of a tile = input k of tied layer j (relu(a_j)),
    the last W rows tanh(a_q) -- the layout the kernels use (tile-major; the [rows, cols] shape is only its size)"""
    rows = disc_act_rows(W, q)
    return act.reshape(-1)[:act.numel()].view(act.shape[1] // 16, rows, 16)


def disc_act_cols(P):
    """columns of that record for P points: whole 16-point tiles"""
    return (P + 15) // 16 * 16


def disc_xproj_rows(W):
    """rows of the x-projection table: the row tiles of the width's kernel (64 for the widths 50 and 64, 96 / 128 for the wide containers)"""
    return 128 if W > 96 else 96 if W > 64 else 64


def disc_xproj(xT, phi, W, out=None):
    """the input layer's x-projection per path, [disc_xproj_rows(W), N] (rows >= W zero): Vin[:, 1..d] x_n + Vin.b -- for disc_fwd(xproj=...)."""
    _need_gpu()
    d, N = xT.shape
    _chk(xT, F64, (d, N), 'xT'); _chk(phi, F64, (phi_size(d, W),), 'phi')
    rows = disc_xproj_rows(W)
    out = torch.empty(rows, N, dtype=F64, device=xT.device) if out is None else out
    _chk(out, F64, (rows, N), 'xproj')
    check(lib.xw_disc_xproj(_p(xT), _p(phi), N, d, W, _p(out), _stream()), 'xw_disc_xproj')
    return out


def disc_fwd(xT, t, phi, W, q, tpp=None, want_vt=True, v=None, vt=None, gxv=None, gtv=None, ngrad=0, max_blocks=0, act=None,
             xproj=None, family=None):
    """v_phi and dv/dt.  Path mode: points (t[l], x_n) -> [L,N].  Point mode (tpp[N]): points (tpp[n], x_n) -> [1,N].
    gxv[d,ngrad] / gtv[ngrad]: also return the input gradient of v at the leading ngrad points (time-major order).
    act[disc_act_rows(W, q), disc_act_cols(L*N)]: also store the layer inputs, for disc_bwd(act=...).
    xproj[disc_xproj_rows(W),N] (path mode, MFMA widths): disc_xproj's table -- the input layer then costs one load per row and point.
    family: 'mfma' / 'tiled' in place of testnet_family(W, q)."""
    family = _disc_family(W, q, family)
    _need_gpu()
    d, N = xT.shape
    L = 1 if tpp is not None else t.shape[0]
    _chk(xT, F64, (d, N), 'xT'); _chk(phi, F64, (phi_size(d, W),), 'phi')
    _chk(t, F64, None, 't'); _chk(tpp, F64, (N,), 'tpp')
    v = torch.empty(L, N, dtype=F64, device=xT.device) if v is None else v
    if want_vt and vt is None:
        vt = torch.empty(L, N, dtype=F64, device=xT.device)
    _chk(v, F64, (L, N), 'v'); _chk(vt, F64, (L, N), 'vt')
    if gxv is not None:
        _chk(gxv, F64, (d, ngrad), 'gxv'); _chk(gtv, F64, (ngrad,), 'gtv')
    if act is not None:
        _chk(act, F64, (disc_act_rows(W, q, family), disc_act_cols(L * N)), 'act')
    if family == 'tiled':
        if xproj is not None:
            raise XnwanError('the tiled test-network family takes no x-projection table')
        check(lib.xw_disc_tiled_fwd(_p(xT), _p(t), _p(tpp), _p(phi), N, L, d, W, q, _p(v), _p(vt if want_vt else None), _p(gxv),
                                    _p(gtv), int(ngrad), int(max_blocks), _p(act), None, _stream()), 'xw_disc_tiled_fwd')
        return v, (vt if want_vt else None)
    if xproj is not None:
        _chk(xproj, F64, (disc_xproj_rows(W), N), 'xproj')
    check(lib.xw_disc_fwd_xproj(_p(xT), _p(t), _p(tpp), _p(phi), N, L, d, W, q, _p(v), _p(vt if want_vt else None), _p(gxv),
                                _p(gtv), int(ngrad), int(max_blocks), _p(act), _p(xproj), _stream()), 'xw_disc_fwd')
    return v, (vt if want_vt else None)


def disc_gradx(xT, t, phi, W, q, tpp=None, vbar=None, gxv=None, gtv=None, family=None):
    """input gradient of <vbar, v>: (nabla_x)[d,N] and (d/dt)[N] at the points (tpp[n] or t[0], x_n); vbar None = ones."""
    family = _disc_family(W, q, family)
    _need_gpu()
    d, N = xT.shape
    _chk(xT, F64, (d, N), 'xT'); _chk(phi, F64, (phi_size(d, W),), 'phi'); _chk(t, F64, None, 't'); _chk(tpp, F64, (N,), 'tpp')
    gxv = torch.empty(d, N, dtype=F64, device=xT.device) if gxv is None else gxv
    gtv = torch.empty(N, dtype=F64, device=xT.device) if gtv is None else gtv
    _chk(gxv, F64, (d, N), 'gxv'); _chk(gtv, F64, (N,), 'gtv')
    if vbar is not None:
        vbar = vbar.reshape(-1)
        _chk(vbar, F64, (N,), 'vbar')
    if family == 'tiled' or not disc_recompute(W, q):
        # other depths / widths: the forward kernel's fused input gradient (any q <= 16; the tiled family: q <= 32), scaled by
        # the cotangent
        t0 = t[:1] if tpp is None else None
        disc_fwd(xT, t0, phi, W, q, tpp=tpp, want_vt=False, gxv=gxv, gtv=gtv, ngrad=N, family=family)
        if vbar is not None:
            gxv.mul_(vbar)
            gtv.mul_(vbar)
        return gxv, gtv
    check(lib.xw_disc_gradx(_p(xT), _p(t), _p(tpp), _p(phi), _p(vbar), N, d, W, q, _p(gxv), _p(gtv), _stream()), 'xw_disc_gradx')
    return gxv, gtv


def disc_bwd_slabs(N, L):
    return lib.xw_disc_bwd_slabs(N, L)


def disc_bwd(xT, t, phi, vbar, W, q, tpp=None, gslab=None, act=None, family=None):
    """parameter gradient of <vbar, v> as partial slabs [nslab, P_v].  act: the record disc_fwd stored for the same phi and
    points (skips the forward recompute)."""
    family = _disc_family(W, q, family)
    _need_gpu()
    d, N = xT.shape
    L = 1 if tpp is not None else t.shape[0]
    P = phi_size(d, W)
    _chk(xT, F64, (d, N), 'xT'); _chk(phi, F64, (P,), 'phi'); _chk(vbar, F64, (L, N), 'vbar')
    _chk(t, F64, None, 't'); _chk(tpp, F64, (N,), 'tpp')
    ns = disc_bwd_slabs(N, L)
    gslab = torch.empty(ns, P, dtype=F64, device=xT.device) if gslab is None else gslab
    _chk(gslab, F64, (ns, P), 'gslab')
    if act is None and (family == 'tiled' or not disc_recompute(W, q)):
        # the recomputing kernel exists at the reference's width and depth only: store the record first, then reverse from it
        act = torch.empty(disc_act_rows(W, q, family), disc_act_cols(L * N), dtype=F64, device=xT.device)
        disc_fwd(xT, t, phi, W, q, tpp=tpp, want_vt=False, act=act, family=family)
    if act is not None:
        _chk(act, F64, (disc_act_rows(W, q, family), disc_act_cols(L * N)), 'act')
    if family == 'tiled':
        check(lib.xw_disc_tiled_bwd(_p(xT), _p(t), _p(tpp), _p(phi), _p(vbar), N, L, d, W, q, _p(act), _p(gslab), _stream()),
              'xw_disc_tiled_bwd')
        return gslab
    check(lib.xw_disc_bwd(_p(xT), _p(t), _p(tpp), _p(phi), _p(vbar), N, L, d, W, q, _p(act), _p(gslab), _stream()),
          'xw_disc_bwd')
    return gslab


def reduce_work_size():
    return lib.xw_reduce_work_size()


def weak_partials(u, v, vt, w, f, h, Vol, Nglob, scal, work, s3x=None, contract=None, c=None, ckappa=0.0, wt=None,
                  finalize=None, pair=None, bdry=None):
    """partial sums of I, sum v^2, SSE_init.  Either s3x[N] (pre-contracted gradient term) or contract = dict(gx, gs, ghT,
    gxv, w0, gwx0T) for the in-kernel contraction with a = identity, b = 0.
    finalize = dict(Lb, Nbglob, alpha, step[, init_off, bdry_off]) (single GPU): also turn the sums into the loss values
    and advance `step`, exactly what losses() does.
    pair = dict(href[N], s3_scale) (L == 1 only): the reference's [N,N] broadcast on a single-slice T0 group, factorised
    (include/xnwan.h); f must then hold mean(f) in every entry.
    bdry = dict(ub[Lb, Nb], g[Lb, Nb]): also add the boundary sum of squares sum (u_b - g)^2 to scal[3] (bdry_partials' sum, same launch)."""
    _need_gpu()
    L, N = u.shape
    for name, a in (('u', u), ('v', v), ('vt', vt), ('f', f)):
        _chk(a, F64, (L, N), name)
    per_point = 1 if w.dim() == 2 else 0
    _chk(w, F64, (L, N) if per_point else (N,), 'w'); _chk(wt, F64, (L, N), 'wt'); _chk(c, F64, (L, N), 'c')
    _chk(s3x, F64, (N,), 's3x'); _chk(h, F64, (N,), 'h'); _chk(scal, F64, (16,), 'scal')
    _chk(work, F64, (reduce_work_size(),), 'work')
    fz = finalize or {}
    _chk(fz.get('step'), torch.int64, (1,), 'step')
    bd, Pb = bdry or {}, 0
    if bdry is not None:
        Pb = bdry['ub'].numel()
        _chk(bdry['ub'], F64, tuple(bdry['ub'].shape), 'ub'); _chk(bdry['g'], F64, tuple(bdry['ub'].shape), 'g')
    pr = pair or {}
    _chk(pr.get('href'), F64, (N,), 'href')
    if pair is not None and L != 1:
        raise XnwanError('the pairwise form only exists for single-slice groups (L == 1)')
    k, d = {}, 0
    if s3x is None:
        k = contract
        d = k['gx'].shape[0]
        for name in ('gx', 'ghT', 'gxv', 'gwx0T'):
            _chk(k[name], F64, (d, N), name)
        _chk(k['gs'], F64, (N,), 'gs'); _chk(k['w0'], F64, (N,), 'w0')
    check(lib.xw_weak_partials(_p(u), _p(v), _p(vt), _p(w), per_point, _p(wt), _p(s3x), _p(k.get('gx')), _p(k.get('gs')),
                               _p(k.get('ghT')), _p(k.get('gxv')), _p(k.get('w0')), _p(k.get('gwx0T')), d, _p(c),
                               float(ckappa), _p(f), _p(h), _p(pr.get('href')), 0 if pair is None else 1,
                               float(pr.get('s3_scale', 1.0)), N, L, float(Vol), float(Nglob), _p(work), _p(scal),
                               0 if finalize is None else 1, max(int(fz.get('Lb', 1)), 1), float(fz.get('Nbglob', 1.0)),
                               float(fz.get('alpha', 0.0)), float(fz.get('init_off', 0.0)), float(fz.get('bdry_off', 0.0)),
                               _p(fz.get('step')), _p(bd.get('ub')), _p(bd.get('g')), Pb, _stream()),
          'xw_weak_partials')


def pair_fold(scal, Vol, Nglob):
    """scal[0] -= (Vol / Nglob) scal[7] scal[8] (several GPUs: after the all-reduce of the partial sums of a pairwise group)"""
    _need_gpu()
    _chk(scal, F64, (16,), 'scal')
    check(lib.xw_pair_fold(_p(scal), float(Vol), float(Nglob), _stream()), 'xw_pair_fold')


def cube_weight(x, top, bot, w, gwT, w0=None, xT=None):
    """w[N], dw/dx as gwT[d, N] (float64) of the hypercube's distance weight at the float32 points x[N, d] -- the values and the
    gradient Hypercube.func_w / autograd give in float32, widened; optionally w0 (a second copy of w) and xT = x^T as float64"""
    _need_gpu()
    N, d = x.shape
    _chk(x, torch.float32, (N, d), 'x')
    _chk(w, F64, (N,), 'w')
    _chk(gwT, F64, (d, N), 'gwT')
    if w0 is not None:
        _chk(w0, F64, (N,), 'w0')
    if xT is not None:
        _chk(xT, F64, (d, N), 'xT')
    check(lib.xw_cube_weight(_p(x), N, d, float(top), float(bot), _p(w), _p(w0), _p(gwT), _p(xT), _stream()), 'xw_cube_weight')


GATHER_ROWS = 1024        # rows of one xw_gather_fields table (include/xnwan.h)


def gather_fields(table, count, total):
    """dst[i][j][k] = src[i s0 + j s1 + k s2] for every row (src, dst, n0, n1, n2, s0, s1, s2, before) of the int64 device table
    [>= count, 9] (addresses as integers; float64 arrays; dst contiguous): the sample fields of all groups of a list-domain
    sample in one launch (Engine.load_groups_packed)"""
    _need_gpu()
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 9 or not table.is_contiguous() or table.shape[0] < count:
        raise XnwanError('gather table: need a contiguous int64 [>= count, 9] device tensor')
    check(lib.xw_gather_fields(_p(table), int(count), int(total), _stream()), 'xw_gather_fields')


def weak_contract_general(A0, amode, B0, gx, gs, ghT, gxv, w0, gwx0T, v0, s3x):
    """s3x[n] = sum_ij a_ij d_i(phi) d_j(u) + phi sum_i b_i d_i(u) at the first time index for general coefficients.
    amode says what A0 is (never inferred from its shape: [d,d] and [d,N] coincide when N == d):
    0 identity (A0 None), 1 [d,d] one matrix, 2 [d,N] diagonal, 3 [d,d,N] full table at t_0;  B0: None or [d,N]."""
    _need_gpu()
    d, N = gx.shape
    for name, a in (('gx', gx), ('ghT', ghT), ('gxv', gxv), ('gwx0T', gwx0T)):
        _chk(a, F64, (d, N), name)
    for name, a in (('gs', gs), ('w0', w0), ('v0', v0), ('s3x', s3x)):
        _chk(a, F64, (N,), name)
    _chk(B0, F64, (d, N), 'B0')
    amode = int(amode)
    if amode not in (0, 1, 2, 3) or (amode == 0) != (A0 is None):
        raise XnwanError('weak_contract_general: amode %r does not match A0' % (amode,))
    if amode:
        _chk(A0, F64, {1: (d, d), 2: (d, N), 3: (d, d, N)}[amode], 'A0')
    check(lib.xw_weak_contract_general(_p(A0), amode, _p(B0), _p(gx), _p(gs), _p(ghT), _p(gxv), _p(w0), _p(gwx0T), _p(v0), d, N,
                                       _p(s3x), _stream()), 'xw_weak_contract_general')
    return s3x


def bdry_partials(ub, g, alpha, Nbglob, scal, work, ubar_b=None):
    _need_gpu()
    L, Nb = ub.shape
    _chk(ub, F64, (L, Nb), 'ub'); _chk(g, F64, (L, Nb), 'g'); _chk(ubar_b, F64, (L, Nb), 'ubar_b'); _chk(scal, F64, (16,), 'scal')
    _chk(work, F64, (reduce_work_size(),), 'work')
    check(lib.xw_bdry_partials(_p(ub), _p(g), Nb, L, float(alpha), float(Nbglob), _p(ubar_b), _p(work), _p(scal), _stream()),
          'xw_bdry_partials')


def gen_cotangents(u, v, w, h, Vol, Nglob, alpha, ubarA, ubarB, c=None, cp=None, ckappa=0.0, pollution=1.0, scal=None):
    """cotangent bases of the generator loss; pass ubarA=None or ubarB=None to form only one of them"""
    _need_gpu()
    if ubarA is None and ubarB is None:
        raise XnwanError('gen_cotangents: nothing to compute')
    L, N = u.shape
    per_point = 1 if w.dim() == 2 else 0
    _chk(u, F64, (L, N), 'u'); _chk(v, F64, (L, N), 'v'); _chk(w, F64, (L, N) if per_point else (N,), 'w')
    _chk(c, F64, (L, N), 'c'); _chk(cp, F64, (L, N), 'cp'); _chk(h, F64, (N,), 'h')
    _chk(ubarA, F64, (L, N), 'ubarA'); _chk(ubarB, F64, (L, N), 'ubarB'); _chk(scal, F64, (16,), 'scal')
    check(lib.xw_gen_cotangents(_p(u), _p(v), _p(w), per_point, _p(c), _p(cp), float(ckappa), _p(h), N, L, float(Vol),
                                float(Nglob), float(alpha), float(pollution), _p(scal), _p(ubarA), _p(ubarB), _stream()),
          'xw_gen_cotangents')


def disc_cotangent(u, v, w, f, h, Vol, Nglob, scal, vbar, c=None, ckappa=0.0, pollution=1.0, s3_scale=1.0):
    _need_gpu()
    L, N = u.shape
    per_point = 1 if w.dim() == 2 else 0
    _chk(u, F64, (L, N), 'u'); _chk(v, F64, (L, N), 'v'); _chk(w, F64, (L, N) if per_point else (N,), 'w')
    _chk(c, F64, (L, N), 'c'); _chk(f, F64, (L, N), 'f'); _chk(h, F64, (N,), 'h'); _chk(vbar, F64, (L, N), 'vbar')
    _chk(scal, F64, (16,), 'scal')
    check(lib.xw_disc_cotangent(_p(u), _p(v), _p(w), per_point, _p(c), float(ckappa), _p(f), _p(h), N, L, float(Vol),
                                float(Nglob), float(pollution), float(s3_scale), _p(scal), _p(vbar), _stream()), 'xw_disc_cotangent')


def losses(scal, L, Lb, Vol, Nglob, Nbglob, alpha, step=None, init_off=0.0, bdry_off=0.0):
    """loss values from the partial sums; also increments `step` when given (pair with adam(..., bump_step=False))"""
    _need_gpu()
    _chk(scal, F64, (16,), 'scal'); _chk(step, torch.int64, (1,), 'step')
    check(lib.xw_losses(_p(scal), L, max(int(Lb), 1), float(Vol), float(Nglob), float(Nbglob), float(alpha), float(init_off),
                        float(bdry_off), _p(step), _stream()), 'xw_losses')


def adam(param, gslabA, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, gextraA=None, gslabB=None, gextraB=None,
         scal=None, gsum_out=None, bump_step=True, lag=None, lag_range=(0, 0), skip=False):
    """param -= Adam(g),  g = gextraA + sum(gslabA) + coefB (gextraB + sum(gslabB)),  coefB = 2 / scal[0] if scal else 1
    lag (device int64[1]) / lag_range: parameters [lo, hi) count their own steps, step - lag; skip: leave that range
    untouched this time and advance lag (torch's Adam skipping parameters whose .grad is None)"""
    _need_gpu()
    P = param.shape[0]
    _chk(param, F64, (P,), 'param'); _chk(m, F64, (P,), 'm'); _chk(v, F64, (P,), 'v'); _chk(step, torch.int64, (1,), 'step')
    nA = nB = 0
    if gslabA is not None:
        nA = gslabA.shape[0]
        _chk(gslabA, F64, (nA, P), 'gslabA')
    if gslabB is not None:
        nB = gslabB.shape[0]
        _chk(gslabB, F64, (nB, P), 'gslabB')
    _chk(gextraA, F64, (P,), 'gextraA'); _chk(gextraB, F64, (P,), 'gextraB'); _chk(gsum_out, F64, (P,), 'gsum_out')
    _chk(scal, F64, (16,), 'scal'); _chk(lag, torch.int64, (1,), 'lag')
    lo, hi = (int(lag_range[0]), int(lag_range[1])) if lag is not None else (0, 0)
    check(lib.xw_adam(_p(param), _p(gslabA), nA, _p(gextraA), _p(gslabB), nB, _p(gextraB), _p(scal), _p(m), _p(v), _p(step),
                      (1 if bump_step is True else 0 if bump_step is False else int(bump_step)), P,
                      float(lr), float(beta1), float(beta2), float(eps), _p(gsum_out), lo, hi, 1 if skip else 0, _p(lag),
                      _stream()), 'xw_adam')


def slab_sum2(gA, outA, gB, outB):
    """outA = sum of the slabs gA[nA, P], outB = sum of gB[nB, P], one launch"""
    _need_gpu()
    (nA, P), (nB, P2) = gA.shape, gB.shape
    _chk(gA, F64, (nA, P), 'gA'); _chk(gB, F64, (nB, P), 'gB'); _chk(outA, F64, (P,), 'outA'); _chk(outB, F64, (P,), 'outB')
    check(lib.xw_slab_sum2(_p(gA), nA, _p(outA), _p(gB), nB, _p(outB), P, _stream()), 'xw_slab_sum2')


def slab_sum(gslab, out=None, accumulate=False):
    _need_gpu()
    ns, P = gslab.shape
    _chk(gslab, F64, (ns, P), 'gslab')
    out = torch.empty(P, dtype=F64, device=gslab.device) if out is None else out
    _chk(out, F64, (P,), 'out')
    check(lib.xw_slab_sum(_p(gslab), ns, P, 1 if accumulate else 0, _p(out), _stream()), 'xw_slab_sum')
    return out
