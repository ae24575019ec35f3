"""The module autograd surface -- `u_net(X)`, `v_net(XV)`, `.backward()` -- against the oracle: case tables, the driver that runs one
case through nets.XNODE / nets.TestNet, the comparison helpers, and plain-torch stand-ins of the kernel wrappers.  No GPU is needed
to import this file (tests/test_gpu_module_surface.py runs the tables on the device, tests/test_module_surface_host.py on the
stand-ins, with defects planted to show that every comparison can fail).

What is under test is host marshalling: nets._OdeFn / _Dopri5Fn / _DiscFn, XNODE.forward, the four operators of ops.py and Blob.split
-- transposes, dtype casts, .contiguous(), the want_x / want_params switches, the flat gradient routed to strided parameter views.
The kernels behind them have oracle tests of their own; here every case goes through the modules with

  * a random cotangent handed to .backward() as a contiguous tensor, as a stride-0 expand, or as a transposed non-contiguous view,
  * float64 / float32 inputs, on the host / on the device, contiguous / a non-contiguous view of a larger tensor,
  * every requires-grad subset (SUBSETS), each variant compared bit for bit with the full case where the issue is only which
    gradients are asked for.

Tolerances: tests/test_gpu_kernels.py `_close` with its values -- both sides float64 from the same inputs, so only summation order
and tanh's last bits differ: 1e-12 values, 1e-11 input gradients, 1e-10 parameter gradients relative to the largest entry of the whole
gradient.  dopri5: the restatement integrated on the device's accepted grid, at tests/test_gpu_dopri5.py GRID_TOL = 1e-9 (the error
estimate is a sum of terms ~1e4 times larger than itself; its rounding moves the step sizes by up to ~2e-10 relative, see there).
A float32 input receives a float32 gradient: the float64 reference rounded once to float32 lies within one float32 ulp of the rounded
device value, in addition to the family's tolerance; where two contributions are accumulated in the float32 .grad (direct + through the
start value) each is rounded once and so is their sum: three ulps of the largest of them.

A stride-0 cotangent cannot vary along the axis it is expanded over: it varies along the other one (N for even case numbers, L for
odd ones); the other two kinds vary over both.
"""
import contextlib
import os
import random
import sys
import types
from collections import namedtuple

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_dopri5 import GRID_TOL  # noqa: E402
from test_gpu_kernels import _close  # noqa: E402

F64, F32 = torch.float64, torch.float32
U_ORDER = ['IL0_w', 'IL0_b', 'IL2_w', 'IL2_b', 'IL4_w', 'IL4_b', 'Win', 'Win_b', 'Wh', 'Wh_b', 'Wo', 'Wo_b', 'FL_w', 'FL_b']
V_ORDER = ['Vin', 'Vin_b', 'Vh', 'Vh_b', 'Vo', 'Vo_b']
TOL_VALUE, TOL_INPUT, TOL_PARAM = 1e-12, 1e-11, 1e-10
ULP32 = 2.0 ** -23

NS, LS, DS = (1, 15, 17, 33), (2, 5), (1, 3)
COTS = ('contiguous', 'expand', 'transposed')
DTYPES = ('float64', 'float32')
PLACES = ('host', 'device')
LAYOUTS = ('contiguous', 'view')
SUBSETS = ('all', 'x_only', 'params_only', 'one_frozen', 'leaf_twice')      # every case runs every one of them (run_u_case / run_v_case)
FIXED = ('euler', 'midpoint', 'rk4')

# (u_hidden_dim, u_hidden_hidden_dim, u_layers) -> the family and blob widths XNODE.bind must report, and whether the blob is embedded
U_SHAPES = {
    'exact20':   (20, 10, 8, 'mfma', (20, 10), False),
    'embed7':    (7, 3, 2, 'mfma', (20, 10), True),
    'embed12':   (12, 6, 2, 'mfma', (20, 10), True),
    'c32':       (32, 12, 10, 'mfma', (32, 12), False),
    'c64':       (64, 16, 2, 'mfma', (64, 16), False),
    'generic48': (48, 16, 11, 'generic', (48, 16), False),
    'tiled128':  (128, 32, 4, 'tiled', (128, 32), False),
    'tiled33':   (33, 17, 2, 'tiled', (33, 17), False),
    'tiled64':   (64, 32, 3, 'tiled', (64, 32), False),
}
# (v_hidden_dim, v_layers) -> TestNet.family, TestNet.kwidth, embedded
V_SHAPES = {
    'w50':      (50, 9, 'mfma', 50, False),
    'embed11':  (11, 2, 'mfma', 50, True),
    'w64':      (64, 4, 'mfma', 64, False),
    'w128':     (128, 2, 'mfma', 128, False),
    'embed70':  (70, 5, 'mfma', 96, True),           # (the issue's "generic width": bind() embeds it in the 96 container)
    'tiled160': (160, 20, 'tiled', 160, False),
    'tiled129': (129, 17, 'tiled', 129, False),
}
V_KINDS = ('points', 'paths', 'grid4')               # XV of shape [M, d+1], [N, L, d+1], [2, 3, 5, d+1]

UCase = namedtuple('UCase', 'no shape solver adjoint stepper N L d cot dtype place layout')
VCase = namedtuple('VCase', 'no shape kind N L d cot dtype place layout')


def u_pairing(c):
    """the code path a case of the u table belongs to: every one of them meets every cotangent kind (and every subset)"""
    if c.solver == 'dopri5':
        return 'dopri5/' + c.stepper
    if c.solver == 'explicit_adams':
        return 'tiled+adams'
    fam = U_SHAPES[c.shape][3]
    return fam + '+adjoint' if c.adjoint else fam


def v_pairing(c):
    return V_SHAPES[c.shape][2]


def _u_cases():
    rows = [(s, solver, False, None, None) for s in ('exact20', 'embed7', 'c32', 'c64', 'generic48', 'tiled128', 'tiled33') for solver in FIXED]
    rows += [('exact20', 'midpoint', True, None, None), ('embed7', 'rk4', True, None, None), ('c32', 'euler', True, None, None)]
    # explicit_adams: the tiled family at every width; two or three sample times are rk4 start-up steps only, five reach the history term
    rows += [('tiled128', 'explicit_adams', False, None, 5), ('tiled33', 'explicit_adams', False, None, 2), ('exact20', 'explicit_adams', False, None, 5)]
    rows += [(s, 'dopri5', False, 'vector', None) for s in ('exact20', 'embed12', 'c32')]
    rows += [(s, 'dopri5', False, 'tiled', None) for s in ('tiled128', 'tiled33', 'tiled64')]
    rng, seen, out = random.Random(22), {}, []
    for no, (shape, solver, adjoint, stepper, L) in enumerate(rows):
        c = UCase(no, shape, solver, adjoint, stepper, rng.choice(NS), L or rng.choice(LS), rng.choice(DS), None, rng.choice(DTYPES),
                  rng.choice(PLACES), rng.choice(LAYOUTS))
        k = seen[u_pairing(c)] = seen.get(u_pairing(c), -1) + 1
        out.append(c._replace(cot=COTS[k % 3]))
    return out


def _v_cases():
    rng, seen, out = random.Random(23), {}, []
    for no, (shape, kind) in enumerate((s, k) for s in V_SHAPES for k in V_KINDS):
        N = 1 if (shape, kind) == ('w50', 'points') else rng.choice(NS)          # (M = 1 among the point sets)
        c = VCase(no, shape, kind, N, rng.choice(LS), rng.choice(DS), None, rng.choice(DTYPES), rng.choice(PLACES), rng.choice(LAYOUTS))
        k = seen[v_pairing(c)] = seen.get(v_pairing(c), -1) + 1
        out.append(c._replace(cot=COTS[k % 3]))
    return out


U_CASES = _u_cases()
V_CASES = _v_cases()
# a single time slice (L == 1): at T0 (the [N, 1] return) and on the boundary, one network per fixed-grid family and dopri5's Function
SLICE_CASES = [('exact20', 'midpoint', None, 17), ('embed7', 'rk4', None, 15), ('generic48', 'euler', None, 33), ('tiled33', 'midpoint', None, 17),
               ('embed12', 'dopri5', 'vector', 15)]


def case_id(c):
    return '-'.join(str(v) for v in c if v is not None and v is not False)


# ------------------------------------------------------------------------------------------------------------------------------
# networks, inputs, cotangents
# ------------------------------------------------------------------------------------------------------------------------------
def _cfg(H=20, K=10, m=8, W=8, q=1, solver='midpoint', adjoint=False):
    return {'alpha': 1e8, 'u_layers': m, 'u_hidden_dim': H, 'u_hidden_hidden_dim': K, 'v_layers': q, 'v_hidden_dim': W, 'n1': 2, 'n2': 1,
            'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': adjoint, 'solver': solver}


def _setup(d, T0=0.0, T=1.0):
    return {'dim': d, 'N_t': 2, 'N_r': 1, 'N_b': 1, 'T0': T0, 'T': T, 'shape_param': [-1, 1]}


def _weights(cfg, d, seed):
    """(theta, phi) of the oracle for `cfg`, seeded, with non-zero biases so that every bias path is exercised"""
    from oracle import refspec as R
    torch.manual_seed(seed)
    theta, phi = R.init_parameters(cfg, _setup(d))
    for p in list(theta.values()) + list(phi.values()):
        if p.dim() == 1:
            p.copy_(0.3 * torch.randn(p.shape, dtype=F64))
    if cfg['u_layers'] == 1:
        theta['Wh_b'].zero_()
    return theta, phi


def fixed_start(start):
    """a start-value callable that does not depend on x: the start values of this sample"""
    return lambda Z: start.to(Z.device)


def smooth_h(Z):
    """a differentiable start value h(x) (float64 whatever the sample's dtype: the reference sees the same values upcast)"""
    return 0.7 * torch.sin(1.3 * Z[:, 1:].to(F64).sum(1)) + 0.2


def smooth_g(Z):
    """start values on the boundary, g(t, x) for Z [N, 1, d+1] -> [N, 1]"""
    return 0.5 * torch.cos(Z[..., 1:].to(F64).sum(-1)) - 0.3


def build_u(shape, solver, adjoint, stepper, d, device, seed, domain=None, T0=0.0):
    """nets.XNODE with the oracle's seeded weights, bound on `device`: (net, theta, cfg); family / widths / embedding asserted"""
    from oracle import refspec as R
    from xnode_wan_pde_solver_amd import nets
    H, K, m, fam, kdims, embedded = U_SHAPES[shape]
    cfg = _cfg(H, K, m, solver=solver, adjoint=adjoint)
    theta, _ = _weights(cfg, d, seed)
    net = nets.XNODE(H, 1, smooth_h, smooth_g, _setup(d, T0=T0), K, m, domain, solver=solver, adjoint=adjoint)
    if stepper is not None:
        net.dopri5_stepper = stepper
    named = dict(net.named_parameters())
    with torch.no_grad():
        for name, key in R.u_names(m):
            p = named[name[len('module.'):]]
            p.copy_(theta[key].reshape(p.shape))
    net.bind(torch.device(device))
    if solver == 'explicit_adams':
        fam, kdims, embedded = 'tiled', (H, K), False
    assert (net.family, tuple(net.kdims), net.blob.embedded) == (fam, kdims, embedded), (shape, net.family, net.kdims, net.blob.embedded)
    if m == 1:
        theta = {k: v for k, v in theta.items() if k not in ('Wh', 'Wh_b')}
    return net, theta, cfg


def build_v(shape, d, device, seed):
    from xnode_wan_pde_solver_amd import nets
    W, q, fam, kw, embedded = V_SHAPES[shape]
    cfg = _cfg(W=W, q=q)
    _, phi = _weights(cfg, d, seed)
    net = nets.TestNet(cfg, {'dim': d})
    with torch.no_grad():
        net.input.weight.copy_(phi['Vin']); net.input.bias.copy_(phi['Vin_b'])
        net.hidden.weight.copy_(phi['Vh']); net.hidden.bias.copy_(phi['Vh_b'])
        net.output.weight.copy_(phi['Vo']); net.output.bias.copy_(phi['Vo_b'])
    net.bind(torch.device(device))
    assert (net.family, net.kwidth, net.blob.embedded) == (fam, kw, embedded), (shape, net.family, net.kwidth, net.blob.embedded)
    return net, phi, cfg


def _place(values, dtype, place, layout, device):
    """`values` (float64, host) as the case's input: its dtype, on the host or the device, contiguous or a view of a larger tensor"""
    t = values.to(F32 if dtype == 'float32' else F64)
    dev = torch.device(device if place == 'device' else 'cpu')
    if layout == 'contiguous':
        return t.contiguous().to(dev)
    big = torch.full([n + 2 for n in t.shape], 7.25, dtype=t.dtype).to(dev)      # (the slices are taken on the device: .to() would pack them)
    view = big[tuple(slice(1, n + 1) for n in t.shape)]
    view.copy_(t.to(dev))
    return view


def paths(N, L, d, seed, t0=0.0, t1=1.0):
    """[N, L, d+1] float64 paths: L sorted times from t0 to t1 in channel 0, one x per path in [-1, 1]^d"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, d, generator=g, dtype=F64) * 2 - 1
    t, _ = torch.sort(torch.rand(L, generator=g, dtype=F64) * (t1 - t0) + t0)
    t[0] = t0
    if L > 1:
        t[-1] = t1
    return torch.cat((t.view(1, L, 1).expand(N, L, 1), x.view(N, 1, d).expand(N, L, d)), 2).contiguous()


def cotangent(kind, lead, no, device):
    """a random float64 cotangent of shape lead + (1,) on `device`, delivered as `kind` says"""
    g = torch.Generator().manual_seed(1000 + no)
    lead = tuple(lead)
    if kind == 'contiguous':
        return torch.randn(lead + (1,), dtype=F64, generator=g).to(device)
    if kind == 'transposed':
        perm = tuple(reversed(range(len(lead))))
        return torch.randn(tuple(reversed(lead)), dtype=F64, generator=g).to(device).permute(perm).unsqueeze(-1)
    axis = (no + 1) % len(lead)                              # expanded (stride 0) along this axis, random along the others
    base = [1 if a == axis else n for a, n in enumerate(lead)]
    return torch.randn(tuple(base) + (1,), dtype=F64, generator=g).to(device).expand(lead + (1,))


# ------------------------------------------------------------------------------------------------------------------------------
# comparison helpers
# ------------------------------------------------------------------------------------------------------------------------------
def close_input_grad(got, ref, tol, what, like, ulps=1):
    """an input gradient against the float64 reference: `like`'s dtype, device and shape; a float32 one within one float32 ulp of
    the reference entry (rounded once) or, for an accumulated one, `ulps` ulps of the largest entry -- in addition to `tol`"""
    assert got is not None, what + ': no gradient arrived'
    assert got.dtype == like.dtype and got.device == like.device and got.shape == like.shape, \
        '%s: gradient is %s %s %s, the input %s %s %s' % (what, got.dtype, got.device, tuple(got.shape), like.dtype, like.device, tuple(like.shape))
    ref = ref.detach().cpu().to(F64)
    if got.dtype == F64:
        return _close(got, ref, tol, what)
    scale = max(float(ref.abs().max()), 1e-300)
    err = (got.detach().cpu().to(F64) - ref).abs()
    bound = tol * scale + ulps * ULP32 * ref.abs().clamp_min(2.0 ** -126) if ulps == 1 else torch.full_like(ref, tol * scale + ulps * ULP32 * scale)
    worst = float((err - bound).max())
    assert worst <= 0.0, '%s: float32 gradient off by %.3e beyond %d ulp + %.0e of the scale %.3e' % (what, worst, ulps, tol, scale)


def close_param_grads(got, ref, tol, what):
    """every parameter's gradient (shape and all) against the oracle's, relative to the largest entry of the whole gradient"""
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert (g is None) == (r is None), '%s: parameter %d has %s where the oracle has %s' % (
            what, i, 'no gradient' if g is None else 'a gradient', 'none' if r is None else 'one')
        if g is not None:
            assert g.dtype == F64 and tuple(g.shape) == tuple(r.shape), '%s: parameter %d gradient %s %s' % (what, i, g.dtype, tuple(g.shape))
    live = [i for i, r in enumerate(ref) if r is not None]
    if live:
        _close(torch.cat([got[i].detach().cpu().reshape(-1) for i in live]), torch.cat([ref[i].reshape(-1) for i in live]), tol, what)


def same_bits(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.dtype == b.dtype and torch.equal(a, b), '%s: bits differ (max |difference| %.3e)' % (what, float((a.double() - b.double()).abs().max()))


# ------------------------------------------------------------------------------------------------------------------------------
# planted defects (tests/test_module_surface_host.py): every comparison above must be able to fail
# ------------------------------------------------------------------------------------------------------------------------------
DEFECTS = ('cot_transposed', 'last_path_dropped', 'last_time_dropped', 'zeros_for_none', 'frozen_gets_grad', 'gx_channels_swapped', 'wrong_ld')


class _TamperOut(torch.autograd.Function):
    """identity on the module's output whose backward spoils the cotangent on its way into the module's Function"""

    @staticmethod
    def forward(ctx, out, defect):
        ctx.defect = defect
        return out.view_as(out)

    @staticmethod
    def backward(ctx, g):
        if ctx.defect == 'cot_transposed' and g.dim() == 3:      # [N, L, 1] read as if it were laid out [L, N]
            g = g.squeeze(2).t().contiguous().view(g.shape)
        elif ctx.defect == 'last_path_dropped':
            g = g.clone()
            g[-1] = 0
        elif ctx.defect == 'last_time_dropped' and g.dim() == 3:
            g = g.clone()
            g[:, -1] = 0
        return g, None


class _TamperIn(torch.autograd.Function):
    """identity on the module's input whose backward swaps the time channel and the first x channel of the input gradient"""

    @staticmethod
    def forward(ctx, X, defect):
        ctx.defect = defect
        return X.view_as(X)

    @staticmethod
    def backward(ctx, g):
        if ctx.defect == 'gx_channels_swapped':
            g = g.clone()
            g[..., 0], g[..., 1] = g[..., 1].clone(), g[..., 0].clone()
        return g, None


@contextlib.contextmanager
def planted(defect):
    """defects that live inside the package: zeros where None is expected (nets._route), a strided view read with the wrong
    leading dimension (Blob.split)"""
    from xnode_wan_pde_solver_amd import nets
    keep_route, keep_split = getattr(nets, '_route', None), nets.Blob.split
    try:
        if defect == 'zeros_for_none':
            nets._route = lambda net, gflat, L: net.blob.split(gflat)
        if defect == 'wrong_ld':
            nets.Blob.split = lambda self, flat: [self._view(flat, s, sl[0], s[1] if len(s) == 2 else 1) for s, sl in zip(self.shapes, self.slots)]
        yield
    finally:
        nets.Blob.split = keep_split
        if keep_route is not None:
            nets._route = keep_route


# ------------------------------------------------------------------------------------------------------------------------------
# the driver: one forward + backward through a module
# ------------------------------------------------------------------------------------------------------------------------------
def surface(net, X, cot, call, frozen=(), x_grad=True, defect=None, twice=False):
    """out = call(net, X'); out.backward(cot) with X' a leaf that shares X's memory layout.  Returns dict(out, gX, grads, X)."""
    names = [n for n, _ in net.named_parameters()]
    for n, p in net.named_parameters():
        p.grad = None
        p.requires_grad_(n not in frozen)
    Xl = X.detach().requires_grad_(x_grad)
    Xin = _TamperIn.apply(Xl, defect) if defect == 'gx_channels_swapped' else Xl
    out = call(net, Xin)
    res = dict(out=out.detach(), X=Xl, names=names)
    if x_grad or len(frozen) < len(names):
        G = cot(out.shape[:-1], out.device)
        assert G.shape == out.shape
        tampered = _TamperOut.apply(out, defect) if defect in ('cot_transposed', 'last_path_dropped', 'last_time_dropped') else out
        torch.autograd.backward(tampered, G, retain_graph=twice)
        res['G'] = G
        if twice:
            res['first'] = (None if Xl.grad is None else Xl.grad.clone(), [None if p.grad is None else p.grad.clone() for p in net.parameters()])
            torch.autograd.backward(tampered, G)
    if defect == 'frozen_gets_grad':
        for n, p in net.named_parameters():
            if n in frozen:
                p.grad = torch.zeros_like(p)
    res['gX'] = Xl.grad
    res['grads'] = [p.grad for p in net.parameters()]
    for p in net.parameters():
        p.requires_grad_(True)
    return res


def _ref_u(cfg):
    from oracle import refspec as R
    if cfg['solver'] == 'explicit_adams':
        import adams_ref as A
        return A.u_net
    return R.u_net


def oracle_u(theta, cfg, X, start_fn, G, frozen_steps=None):
    """u [N, L] (or [N, 1] for a single slice), d/dX [N, L, d+1] and the parameter gradients of sum(u G) by torch autograd on the
    oracle, float64, from the same values upcast"""
    th = {k: v.clone().requires_grad_(True) for k, v in theta.items()}
    Xo = X.detach().cpu().to(F64).contiguous().clone().requires_grad_(True)
    start = start_fn(Xo[:, 0, :] if start_fn is not smooth_g else Xo[:, :1, :]).reshape(-1)
    if cfg['solver'] == 'dopri5':
        import dopri5_ref as D
        u = D.u_net(th, cfg, Xo, start, frozen=frozen_steps)[0] if Xo.shape[1] > 1 else _ref_u(dict(cfg, solver='euler'))(th, cfg, Xo, start)
    else:
        u = _ref_u(cfg)(th, cfg, Xo, start)
    keys = [k for k in U_ORDER if k in th]
    gs = torch.autograd.grad((u * G.detach().cpu().reshape(u.shape)).sum(), [Xo] + [th[k] for k in keys], allow_unused=True)
    return u.detach(), (gs[0] if gs[0] is not None else torch.zeros_like(Xo)), list(gs[1:])


def _frozen_steps(net, cfg):
    return net.last_dopri5.steps if cfg['solver'] == 'dopri5' else None


def check_u(tag, res, ref, X, tols, ulps=1):
    """one run of the u surface against the oracle: values, the input gradient the way the fixtures took it (x channels of time
    slice 0; everything else exactly zero: this project returns the time channel as zero, nets._OdeFn.backward), every parameter"""
    u_ref, gX_ref, gp_ref = ref
    tv, tx, tp = tols
    out = res['out']
    assert out.dtype == F64 and tuple(out.shape) == tuple(u_ref.shape) + (1,) and out.is_contiguous(), (tag, out.dtype, tuple(out.shape))
    _close(out.squeeze(-1), u_ref, tv, tag + ' u')
    if res['X'].requires_grad:
        gX = res['gX']
        assert gX is not None, tag + ': X received no gradient'
        assert float(gX[:, :, 0].abs().max()) == 0.0, tag + ': the time channel of d/dX is not zero'
        if gX.shape[1] > 1:
            assert float(gX[:, 1:, 1:].abs().max()) == 0.0, tag + ': d/dX beyond time slice 0 is not zero'
        want = torch.zeros_like(gX_ref)
        want[:, 0, 1:] = gX_ref[:, 0, 1:]
        close_input_grad(gX, want, tx, tag + ' d/dX', res['X'], ulps)
    else:
        assert res['gX'] is None, tag + ': X does not require a gradient and has one'
    close_param_grads(res['grads'], gp_ref, tp, tag + ' parameter gradients')


def u_tolerances(solver):
    return (GRID_TOL,) * 3 if solver == 'dopri5' else (TOL_VALUE, TOL_INPUT, TOL_PARAM)


def run_u_case(c, device, defect=None):
    """one row of U_CASES through nets.XNODE on `device`: the full case against the oracle, then every other requires-grad subset
    (bit for bit against the full case where only the set of gradients asked for differs), no_grad, twice, repeated"""
    net, theta, cfg = build_u(c.shape, c.solver, c.adjoint, c.stepper, c.d, device, 300 + c.no)
    X = _place(paths(c.N, c.L, c.d, 400 + c.no), c.dtype, c.place, c.layout, device)
    start = torch.randn(c.N, dtype=F64, generator=torch.Generator().manual_seed(500 + c.no))
    cot = lambda lead, dev: cotangent(c.cot, lead, c.no, dev)          # noqa: E731
    call = lambda n, Z: n(Z, starts_at_T0=True)                        # noqa: E731
    tols, tag = u_tolerances(c.solver), case_id(c)
    names = [n for n, _ in net.named_parameters()]
    with planted(defect):
        net.h = fixed_start(start)
        full = surface(net, X, cot, call, defect=defect)
        steps = _frozen_steps(net, cfg)
        assert full['out'].device == net.blob.data.device
        ref = oracle_u(theta, cfg, X, net.h, full['G'], steps)
        check_u(tag + ' [all]', full, ref, X, tols)
        # the same call with no gradient recorded; repeated; two backward passes over one graph
        with torch.no_grad():
            same_bits(call(net, X.detach()), full['out'], tag + ' forward under no_grad')
        again = surface(net, X, cot, call, twice=True)
        same_bits(again['out'], full['out'], tag + ' repeated: u')
        same_bits(again['first'][0], full['gX'], tag + ' repeated: d/dX')
        for a, b in zip(again['first'][1], full['grads']):
            same_bits(a, b, tag + ' repeated: parameter gradient')
        same_bits(again['gX'], 2 * full['gX'], tag + ' two backward passes: d/dX')
        for a, b in zip(again['grads'], full['grads']):
            same_bits(a, 2 * b, tag + ' two backward passes: parameter gradient')
        # only X: every parameter frozen
        only_x = surface(net, X, cot, call, frozen=names, defect=defect)
        assert all(g is None for g in only_x['grads']), tag + ' [x_only]: a frozen parameter has a gradient'
        want = torch.zeros_like(ref[1])
        want[:, 0, 1:] = ref[1][:, 0, 1:]
        close_input_grad(only_x['gX'], want, tols[1], tag + ' [x_only] d/dX', X)       # (its bits against the full case: x_only_bits)
        assert float(only_x['gX'][:, :, 0].abs().max()) == 0.0
        # only the parameters
        only_p = surface(net, X, cot, call, x_grad=False, defect=defect)
        assert only_p['gX'] is None
        for a, b in zip(only_p['grads'], full['grads']):
            same_bits(a, b, tag + ' [params_only] parameter gradient against the full case')
        # one parameter frozen
        cold = names[(7 * c.no + 3) % len(names)]
        one = surface(net, X, cot, call, frozen=(cold,), defect=defect)
        same_bits(one['gX'], full['gX'], tag + ' [one_frozen] d/dX')
        for n, a, b in zip(names, one['grads'], full['grads']):
            if n == cold:
                assert a is None, tag + ' [one_frozen]: the frozen parameter %s has a gradient' % n
            else:
                same_bits(a, b, tag + ' [one_frozen] gradient of ' + n)
        # X as a leaf that the gradient reaches twice: through the start value h(x) and directly
        net.h = smooth_h
        leaf = surface(net, X, cot, call, defect=defect)
        check_u(tag + ' [leaf_twice]', leaf, oracle_u(theta, cfg, X, smooth_h, leaf['G'], _frozen_steps(net, cfg)), X, tols, ulps=3)
    return net


def x_only_bits(c, device):
    """d/dX with every parameter frozen (the sweep runs without want_params) and d/dX of the full case: (the two tensors, the number
    of entries whose bits differ, the largest |difference| relative to the largest entry)"""
    net, _, _ = build_u(c.shape, c.solver, c.adjoint, c.stepper, c.d, device, 300 + c.no)
    X = _place(paths(c.N, c.L, c.d, 400 + c.no), c.dtype, c.place, c.layout, device)
    net.h = fixed_start(torch.randn(c.N, dtype=F64, generator=torch.Generator().manual_seed(500 + c.no)))
    cot = lambda lead, dev: cotangent(c.cot, lead, c.no, dev)          # noqa: E731
    call = lambda n, Z: n(Z, starts_at_T0=True)                        # noqa: E731
    full = surface(net, X, cot, call)['gX']
    only = surface(net, X, cot, call, frozen=[n for n, _ in net.named_parameters()])['gX']
    diff = (full.double() - only.double()).abs()
    return full, only, int((full != only).sum()), float(diff.max()) / max(float(full.double().abs().max()), 1e-300)


def run_slice_case(shape, solver, stepper, N, device, boundary, defect=None):
    """L == 1: at T0 the [N, 1] return with the oracle's values, on the boundary [N, 1, 1] from g; the lift's and read-out's gradients
    are the oracle's, the field's are None (no step was taken: the reference never puts ODE_rhs in the graph)"""
    d = 3
    net, theta, cfg = build_u(shape, solver, False, stepper, d, device, 600 + N)
    X = paths(N, 1, d, 601 + N, t0=0.4 if boundary else 0.0).to(F32).to(device)
    tag = '%s %s single slice %s' % (shape, solver, 'on the boundary' if boundary else 'at T0')
    cot = lambda lead, dev: cotangent('contiguous', lead, N, dev)       # noqa: E731
    names = [n for n, _ in net.named_parameters()]
    with planted(defect):
        if boundary:
            res = surface(net, X, cot, lambda n, Z: n(Z, starts_at_T0=False), defect=defect)
            assert tuple(res['out'].shape) == (N, 1, 1), tag
            ref = oracle_u(theta, cfg, X, smooth_g, res['G'])
        else:
            res = surface(net, X, cot, lambda n, Z: n(Z).unsqueeze(2), defect=defect)       # (looked up: X[0, 0, 0] == T0)
            assert tuple(net(X.detach()).shape) == (N, 1), tag + ': the reference returns [N, 1] here'
            ref = oracle_u(theta, cfg, X, smooth_h, res['G'])
    for n, g in zip(names, ref[2]):
        assert (g is None) == n.startswith('ODE_rhs.'), n            # (the oracle itself: autograd never reaches the field)
    check_u(tag, res, ref, X, u_tolerances('euler'), ulps=1)
    return res


# ---- v_net -----------------------------------------------------------------------------------------------------------------------
def smooth_w(XV):
    return torch.cos(0.9 * XV[..., 1:].to(F64).sum(-1)) + 0.1 * XV[..., 0].to(F64)


def v_points(c, seed):
    g = torch.Generator().manual_seed(seed)
    shape = {'points': (c.N,), 'paths': (c.N, c.L), 'grid4': (2, 3, 5)}[c.kind]
    XV = torch.rand(shape + (c.d + 1,), generator=g, dtype=F64) * 2 - 1
    XV[..., 0] = XV[..., 0].abs()
    return XV


def oracle_v(phi, cfg, XV, G, weight=None):
    from oracle import refspec as R
    ph = {k: v.clone().requires_grad_(True) for k, v in phi.items()}
    Xo = XV.detach().cpu().to(F64).contiguous().clone().requires_grad_(True)
    v = R.v_net(ph, cfg, Xo)
    out = v if weight is None else v * weight(Xo)
    gs = torch.autograd.grad((out * G.detach().cpu().reshape(out.shape)).sum(), [Xo] + [ph[k] for k in V_ORDER])
    return v.detach(), gs[0], list(gs[1:])


def check_v(tag, res, ref, ulps=1):
    v_ref, gX_ref, gp_ref = ref
    out = res['out']
    assert out.dtype == F64 and tuple(out.shape) == tuple(v_ref.shape) + (1,) and out.is_contiguous(), (tag, out.dtype, tuple(out.shape))
    _close(out.squeeze(-1), v_ref, TOL_VALUE, tag + ' v')
    if res['X'].requires_grad:
        close_input_grad(res['gX'], gX_ref, TOL_INPUT, tag + ' d/dXV (time channel included)', res['X'], ulps)
    else:
        assert res['gX'] is None
    close_param_grads(res['grads'], gp_ref, TOL_PARAM, tag + ' parameter gradients')


def run_v_case(c, device, defect=None):
    net, phi, cfg = build_v(c.shape, c.d, device, 700 + c.no)
    XV = _place(v_points(c, 800 + c.no), c.dtype, c.place, c.layout, device)
    cot = lambda lead, dev: cotangent(c.cot, lead, c.no, dev)          # noqa: E731
    call = lambda n, Z: n(Z)                                           # noqa: E731
    tag = case_id(c)
    names = [n for n, _ in net.named_parameters()]
    with planted(defect):
        full = surface(net, XV, cot, call, defect=defect)
        assert full['out'].device == net.blob.data.device
        check_v(tag + ' [all]', full, oracle_v(phi, cfg, XV, full['G']))
        with torch.no_grad():
            same_bits(call(net, XV.detach()), full['out'], tag + ' forward under no_grad')
        again = surface(net, XV, cot, call, twice=True)
        same_bits(again['out'], full['out'], tag + ' repeated: v')
        same_bits(again['first'][0], full['gX'], tag + ' repeated: d/dXV')
        for a, b in zip(again['first'][1], full['grads']):
            same_bits(a, b, tag + ' repeated: parameter gradient')
        same_bits(again['gX'], 2 * full['gX'], tag + ' two backward passes: d/dXV')
        for a, b in zip(again['grads'], full['grads']):
            same_bits(a, 2 * b, tag + ' two backward passes: parameter gradient')
        only_x = surface(net, XV, cot, call, frozen=names, defect=defect)
        assert all(g is None for g in only_x['grads']), tag + ' [x_only]: a frozen parameter has a gradient'
        same_bits(only_x['gX'], full['gX'], tag + ' [x_only] d/dXV against the full case')
        only_p = surface(net, XV, cot, call, x_grad=False, defect=defect)
        for a, b in zip(only_p['grads'], full['grads']):
            same_bits(a, b, tag + ' [params_only] parameter gradient against the full case')
        cold = names[(5 * c.no + 2) % len(names)]
        one = surface(net, XV, cot, call, frozen=(cold,), defect=defect)
        same_bits(one['gX'], full['gX'], tag + ' [one_frozen] d/dXV')
        for n, a, b in zip(names, one['grads'], full['grads']):
            if n == cold:
                assert a is None, tag + ' [one_frozen]: the frozen parameter %s has a gradient' % n
            else:
                same_bits(a, b, tag + ' [one_frozen] gradient of ' + n)
        # XV as a leaf reached twice: through v and through a differentiable weight w(XV) -- phi = v w, as the loss forms it
        leaf = surface(net, XV, cot, lambda n, Z: n(Z) * smooth_w(Z).to(n.blob.data.device).unsqueeze(-1), defect=defect)
        ref = oracle_v(phi, cfg, XV, leaf['G'], weight=smooth_w)
        leaf['out'] = full['out']
        check_v(tag + ' [leaf_twice]', leaf, ref, ulps=3)
    return net


# ------------------------------------------------------------------------------------------------------------------------------
# plain-torch stand-ins of the kernel wrappers (the CPU tests): the modules, their Functions and the operators stay the real ones
# ------------------------------------------------------------------------------------------------------------------------------
def _with_autograd(fn):
    """run fn in a thread of its own with gradients enabled: inside a custom operator the autograd dispatch keys are excluded for
    the calling thread, so a plain-torch stand-in that differentiates the oracle there needs a fresh thread state"""
    import functools
    import threading

    @functools.wraps(fn)
    def run(*a, **kw):
        box = {}

        def body():
            try:
                with torch.enable_grad():
                    box['out'] = fn(*a, **kw)
            except BaseException as exc:       # noqa: B036  (re-raised in the caller)
                box['exc'] = exc
        th = threading.Thread(target=body)
        th.start()
        th.join()
        if 'exc' in box:
            raise box['exc']
        return box['out']
    return run


def _u_views(flat, d, H, K):
    """the oracle's parameter dict as views of a blob laid out at the widths (H, K) (include/xnwan.h; nets._u_slots)"""
    from xnode_wan_pde_solver_amd import nets
    slots, total = nets._u_slots(d, H, K, H, K, True)
    assert flat.numel() == total
    shapes = [(H, 1), (H,), (H, H), (H,), (H, H), (H,), (K, d + 1 + H), (K,), (K, K), (K,), (H, K), (H,), (1, H), (1,)]
    return {k: nets.Blob._view(flat, s, sl[0], sl[3]) for k, s, sl in zip(U_ORDER, shapes, slots)}


def _v_views(flat, d, W):
    from xnode_wan_pde_solver_amd import nets
    slots, total = nets._v_slots(d, W, W)
    assert flat.numel() == total
    shapes = [(W, d + 1), (W,), (W, W), (W,), (1, W), (1,)]
    return {k: nets.Blob._view(flat, s, sl[0], sl[3]) for k, s, sl in zip(V_ORDER, shapes, slots)}


def _pack(views_of, grads, order, total):
    flat = torch.zeros(total, dtype=F64)
    for k, g in zip(order, grads):
        if g is not None:
            views_of(flat)[k].copy_(g)
    return flat


def _solver_name(method):
    from xnode_wan_pde_solver_amd import kernels as KN
    if method == KN.ADAMS:
        return 'explicit_adams'
    return {v: k for k, v in KN.METHODS.items()}[method]


def _X_of(xT, t):
    d, N = xT.shape
    L = t.shape[0]
    return torch.cat((t.view(1, L, 1).expand(N, L, 1), xT.t().reshape(N, 1, d).expand(N, L, d)), 2)


@_with_autograd
def _u_sweep(xT, t, start, theta, ubar, cfg, H, K, want_params, frozen=None):
    d, N = xT.shape
    th = {k: v.clone().requires_grad_(True) for k, v in _u_views(theta, d, H, K).items()}
    x = xT.clone().requires_grad_(True)
    s = start.clone().requires_grad_(True)
    if cfg['solver'] == 'dopri5' and t.shape[0] > 1:
        import dopri5_ref as D
        u = D.u_net(th, cfg, _X_of(x, t), s, frozen=frozen)[0]
    else:
        u = _ref_u(cfg if cfg['solver'] != 'dopri5' else dict(cfg, solver='euler'))(th, cfg, _X_of(x, t), s)
    gs = torch.autograd.grad((u * ubar.t()).sum(), [x, s] + [th[k] for k in U_ORDER], allow_unused=True)
    gx = gs[0] if gs[0] is not None else torch.zeros_like(xT)
    flat = _pack(lambda f: _u_views(f, d, H, K), gs[2:], U_ORDER, theta.numel()) if want_params else None
    return gx.contiguous(), gs[1], flat


@contextlib.contextmanager
def standin():
    """kernels.family_ode_fwd / family_ode_bwd / dopri5_fwd / dopri5_sweep / disc_fwd / disc_gradx / disc_bwd / slab_sum replaced by
    plain torch on the oracle (R.u_net, R.v_net, tests/adams_ref.py, tests/dopri5_ref.py), same signatures and layouts, any device"""
    from oracle import refspec as R
    from xnode_wan_pde_solver_amd import kernels as KN

    def family_ode_fwd(xT, t, start, theta, method, H, K, m, want_Y=True, family=None):
        cfg = _cfg(H, K, m, solver=_solver_name(method))
        with torch.no_grad():
            u = _ref_u(cfg)(_u_views(theta, xT.shape[0], H, K), cfg, _X_of(xT, t), start)
        return u.t().contiguous(), (torch.zeros(t.shape[0], H, xT.shape[1], dtype=F64) if want_Y else None)

    def family_ode_bwd(xT, t, start, theta, Y, ubar, method, H, K, m, want_x=True, want_params=False, adjoint=False, family=None):
        cfg = _cfg(H, K, m, solver=_solver_name(method), adjoint=adjoint)
        gx, gs, flat = _u_sweep(xT, t, start, theta, ubar, cfg, H, K, want_params)
        return gx, gs, (flat.view(1, -1) if want_params else None)

    def dopri5_fwd(jobs, t, theta, H, K, m, Hn, rtol=KN.DOPRI5_RTOL, atol=KN.DOPRI5_ATOL, stepper='vector', **_):
        import dopri5_ref as D
        cfg, recs = _cfg(H, K, m, solver='dopri5'), []
        for j in jobs:
            th = _u_views(theta, j['xT'].shape[0], H, K)
            with torch.no_grad():
                if t.shape[0] > 1:
                    u, info = D.u_net(th, cfg, _X_of(j['xT'], t), j['start'], rtol=rtol, atol=atol)
                else:
                    u, info = R.u_net(th, cfg, _X_of(j['xT'], t), j['start']), {'steps': []}
            j['u'].copy_(u.t())
            recs.append(types.SimpleNamespace(steps=list(info['steps']), stepper=stepper))
        return recs

    def dopri5_sweep(jobs, t, theta, H, K, m, want_x, want_params, x_cot_ones=False, stepper='vector'):
        cfg = _cfg(H, K, m, solver='dopri5')
        for j in jobs:
            gx, gs, flat = _u_sweep(j['xT'], t, j['start'], theta, j['ubar'], cfg, H, K, want_params, frozen=j['rec'].steps)
            j['gx'].copy_(gx), j['gs'].copy_(gs)
            if want_params:
                j['gslab'].zero_()
                j['gslab'][0].copy_(flat)

    def _pts(xT, tpp):
        return torch.cat((tpp.view(-1, 1), xT.t()), 1)

    def disc_fwd(xT, t, phi, W, q, tpp=None, want_vt=True, **_):
        assert t is None and not want_vt
        with torch.no_grad():
            return R.v_net(_v_views(phi, xT.shape[0], W), {'v_layers': q}, _pts(xT, tpp)).view(1, -1), None

    @_with_autograd
    def disc_gradx(xT, t, phi, W, q, tpp=None, vbar=None, **_):
        pts = _pts(xT, tpp).clone().requires_grad_(True)
        g, = torch.autograd.grad((R.v_net(_v_views(phi, xT.shape[0], W), {'v_layers': q}, pts) * vbar.view(-1)).sum(), [pts])
        return g[:, 1:].t().contiguous(), g[:, 0].contiguous()

    @_with_autograd
    def disc_bwd(xT, t, phi, vbar, W, q, tpp=None, **_):
        d = xT.shape[0]
        ph = {k: v.clone().requires_grad_(True) for k, v in _v_views(phi, d, W).items()}
        gs = torch.autograd.grad((R.v_net(ph, {'v_layers': q}, _pts(xT, tpp)) * vbar.view(-1)).sum(), [ph[k] for k in V_ORDER], allow_unused=True)
        return _pack(lambda f: _v_views(f, d, W), gs, V_ORDER, phi.numel()).view(1, -1)

    new = dict(family_ode_fwd=family_ode_fwd, family_ode_bwd=family_ode_bwd, dopri5_fwd=dopri5_fwd, dopri5_sweep=dopri5_sweep,
               disc_fwd=disc_fwd, disc_gradx=disc_gradx, disc_bwd=disc_bwd, slab_sum=lambda gslab, out=None, accumulate=False: gslab.sum(0))
    keep = {k: getattr(KN, k) for k in new}
    try:
        for k, f in new.items():
            setattr(KN, k, f)
        yield
    finally:
        for k, f in keep.items():
            setattr(KN, k, f)


# ------------------------------------------------------------------------------------------------------------------------------
# the evaluation path (bound_pad) with gradients, and the refusals
# ------------------------------------------------------------------------------------------------------------------------------
def run_bound_pad_case(device):
    """paths on the cube that start neither at T0 nor on the boundary: XNODE.forward integrates from the first slice's g over
    domain.bound_pad's densified grid and gathers the requested times; the reference is the oracle on the padded grid.  Parameter
    gradients flow through the gather, x's through the repeated first slice and through g."""
    from oracle import refspec as R
    from xnode_wan_pde_solver_amd.sampling import Hypercube
    N, d = 17, 3
    domain = Hypercube([-1, 1], d, 0.0, 1.0, 6)
    net, theta, cfg = build_u('exact20', 'midpoint', False, None, d, device, 900, domain=domain)
    X = paths(N, 3, d, 901) * 0.8
    X[:, :, 0] = torch.tensor([0.33, 0.61, 0.97], dtype=F64).view(1, 3)
    X = X.to(device)
    res = surface(net, X, lambda lead, dev: cotangent('transposed', lead, 5, dev), lambda n, Z: n(Z))
    _, gather, filled = domain.bound_pad(X.detach().cpu())
    grid = filled.to(F64)
    assert grid.shape[0] > 3 and float(grid[0]) == 0.0 and tuple(res['out'].shape) == (N, 3, 1)
    th = {k: v.clone().requires_grad_(True) for k, v in theta.items()}
    Xo = X.detach().cpu().clone().requires_grad_(True)
    Xp = torch.cat((grid.view(1, -1, 1).expand(N, -1, 1), Xo[:, :1, 1:].expand(-1, grid.shape[0], -1)), 2)
    u = R.u_net(th, cfg, Xp, smooth_g(Xo[:, :1, :]).reshape(-1))[:, gather.long()]
    keys = [k for k in U_ORDER if k in th]
    gs = torch.autograd.grad((u * res['G'].detach().cpu().squeeze(2)).sum(), [Xo] + [th[k] for k in keys])
    check_u('bound_pad on the cube', res, (u.detach(), gs[0], list(gs[1:])), X, (TOL_VALUE, TOL_INPUT, TOL_PARAM))


def check_refusals(device):
    """what the surface refuses, with the messages it refuses them with"""
    import pytest
    from xnode_wan_pde_solver_amd import nets
    from xnode_wan_pde_solver_amd._lib import XnwanError
    from xnode_wan_pde_solver_amd.sampling import Hypercube
    d = 3
    with pytest.raises(XnwanError, match="solver 'dopri5' with adjoint=True is not served"):
        nets.XNODE(20, 1, smooth_h, smooth_g, _setup(d), 10, 8, None, solver='dopri5', adjoint=True)
    with pytest.raises(XnwanError, match="solver 'explicit_adams' with adjoint=True is not served"):
        nets.XNODE(20, 1, smooth_h, smooth_g, _setup(d), 10, 8, None, solver='explicit_adams', adjoint=True)
    X = (paths(5, 3, d, 902) * 0.8).to(F32)
    with pytest.raises(XnwanError, match=r'XNODE.bind\(device\) has not been called'):
        nets.XNODE(20, 1, smooth_h, smooth_g, _setup(d), 10, 8, None)(X)
    with pytest.raises(XnwanError, match=r'TestNet.bind\(device\) has not been called'):
        nets.TestNet(_cfg(W=50, q=9), {'dim': d})(X)
    net, _, _ = build_u('exact20', 'dopri5', False, 'vector', d, device, 903, domain=Hypercube([-1, 1], d, 0.0, 1.0, 6))
    Xe = X.clone()
    Xe[:, :, 0] = torch.tensor([0.33, 0.61, 0.97]).view(1, 3)
    with pytest.raises(XnwanError, match="solver 'dopri5': paths that start neither at T0 nor on the boundary"):
        net(Xe)
    for net in (build_u('exact20', 'midpoint', False, None, d, device, 904)[0], build_v('w50', d, device, 905)[0]):
        p = next(net.parameters())
        p.data = p.data.clone()
        with pytest.raises(XnwanError, match='a parameter no longer aliases its blob'):
            net(X, starts_at_T0=True) if isinstance(net, nets.XNODE) else net(X)
