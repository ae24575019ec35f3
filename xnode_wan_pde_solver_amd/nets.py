"""Network shells: nn.Modules with the reference's attribute names / state_dict keys whose parameters are VIEWS into
one flat float64 blob per network -- the blob is what the HIP kernels read and what the fused Adam kernel updates.

Call surface mirrored (file:line into the reference):
    XNODE            <- NeuralODE        src/model.py:54-112      u_theta: lift h/g -> hidden state, fixed-grid ODE, read-out
    HiddenField      <- _ODEField        src/model.py:115-141     the field MLP (one weight-tied hidden Linear)
    TestNet          <- discriminator    src/model.py:18-51       v_phi (one weight-tied hidden Linear)
    PathParallel     <- nn.DataParallel  src/training.py:93-97    only the `.module` wrapper / `module.` key prefix; the
                                                                  actual multi-GPU strategy is in dist.py
    init_weights                          src/model.py:12-15
Module construction order and `apply(init_weights)` order are the reference's, so seeded runs draw identical weights
(pinned by tests/golden).

The modules' forward()/backward run on the HIP kernels through two autograd Functions, so `u_net(X)`, `v_net(XV)`,
`.backward()` and torch optimisers keep working for user code; the training loop itself does not use autograd at all
(engine.py).
"""
import torch
from torch import nn

from . import kernels as KN
from . import ops as _ops  # noqa: F401  (registers the xnwan:: operators)
from ._lib import XnwanError

F64 = torch.float64


def init_weights(layer):
    """Xavier-uniform weights, zero bias on every Linear (reference src/model.py:12-15)."""
    if type(layer) == nn.Linear:
        nn.init.xavier_uniform_(layer.weight)
        layer.bias.data.fill_(0)


# ----------------------------------------------------------------------------------------------------------------------
# flat parameter storage
# ----------------------------------------------------------------------------------------------------------------------
class Blob:
    """One contiguous float64 vector holding all parameters of a network in the kernels' layout (include/xnwan.h:
    named_parameters() order, row-major matrices) -- at the width of the kernel instantiation the network runs in.

    `slots`: for every parameter of named_parameters() its place in the blob, (offset, rows, cols, leading dimension[,
    column offset]); missing slots (a field without hidden layer, u_layers = 1) stay zero.  When the network is as wide as
    the instantiation the parameters are contiguous pieces; a narrower network is EMBEDDED: every matrix is the leading
    block of its zero-padded container (the y-columns of Win keep their place behind x and t), so the module's parameters
    become strided views and the padding never leaves zero (kernels.ODE_WIDTHS)."""

    def __init__(self, module, device, slots=None, total=None):
        params = [p for _, p in module.named_parameters()]      # de-duplicated: tied layers appear once
        self.names = [n for n, _ in module.named_parameters()]
        self.shapes = [tuple(p.shape) for p in params]
        self.sizes = [p.numel() for p in params]
        if slots is None:                                       # plain concatenation
            slots, off = [], 0
            for p in params:
                r, c = (p.shape[0], p.shape[1]) if p.dim() == 2 else (1, p.numel())
                slots.append((off, r, c, c))
                off += p.numel()
            total = off
        self.data = torch.zeros(total, dtype=F64, device=device)
        self.grad = torch.zeros_like(self.data)
        self.slots = slots
        self.offsets = [sl[0] for sl in slots]
        for p, (off, r, c, ld) in zip(params, slots):
            if p.dtype != F64:
                raise XnwanError('network parameters must be float64 (the reference computes in float64 throughout)')
            view = self._view(self.data, p.shape, off, ld)
            view.copy_(p.data)
            p.data = view                                       # parameter now aliases the blob
        self.params = params
        self.embedded = any(p.dim() == 2 and sl[3] != p.shape[1] for p, sl in zip(params, slots)) or total != sum(self.sizes)

    @staticmethod
    def _view(flat, shape, off, ld):
        if len(shape) == 2:
            return flat.as_strided(tuple(shape), (ld, 1), flat.storage_offset() + off)     # (as_strided's offset is absolute)
        return flat[off:off + shape[0]]

    def split(self, flat):
        """the per-parameter pieces of a vector laid out like the blob (a gradient), as tensors of the parameters' shapes"""
        return [self._view(flat, s, sl[0], sl[3]) for s, sl in zip(self.shapes, self.slots)]

    def check_alias(self):
        """The kernels read the blob, user code sees the Parameters: make sure they are still the same memory."""
        for p, o in zip(self.params, self.offsets):
            if p.data.data_ptr() != self.data.data_ptr() + 8 * o:
                raise XnwanError('a parameter no longer aliases its blob (module moved/cast after construction?) -- '
                                 'call solver.rebind() after .to()/.double()')


def _u_slots(d, H, K, Hc, Kc, has_hidden):
    """places of u_theta's parameters (named_parameters() order) in the blob of width (Hc, Kc); include/xnwan.h layout"""
    ldin, p = d + 1 + Hc, 0
    sl = []
    for r, c, rc, cc in ((H, 1, Hc, 1), (H, None, Hc, None), (H, H, Hc, Hc), (H, None, Hc, None), (H, H, Hc, Hc), (H, None, Hc, None)):
        sl.append((p, r, c if c else 1, cc if cc else 1))       # IL0.w, IL0.b, IL2.w, IL2.b, IL4.w, IL4.b
        p += rc * (cc if cc else 1)
    sl.append((p, K, d + 1 + H, ldin)); p += Kc * ldin          # Win (x | t | y columns: the y block keeps its offset d + 1)
    sl.append((p, K, 1, 1)); p += Kc                            # Win.b
    if has_hidden:
        sl.append((p, K, K, Kc))
    p += Kc * Kc                                                # Wh (slot kept zero when the field has no hidden layer)
    if has_hidden:
        sl.append((p, K, 1, 1))
    p += Kc
    sl.append((p, H, K, Kc)); p += Hc * Kc                      # Wo
    sl.append((p, H, 1, 1)); p += Hc                            # Wo.b
    sl.append((p, 1, H, Hc)); p += Hc                           # FL.w
    sl.append((p, 1, 1, 1)); p += 1                             # FL.b
    return sl, p


def _v_slots(d, W, Wc):
    p, sl = 0, []
    sl.append((p, W, d + 1, d + 1)); p += Wc * (d + 1)          # Vin
    sl.append((p, W, 1, 1)); p += Wc
    sl.append((p, W, W, Wc)); p += Wc * Wc                      # Vh
    sl.append((p, W, 1, 1)); p += Wc
    sl.append((p, 1, W, Wc)); p += Wc                           # Vo
    sl.append((p, 1, 1, 1)); p += 1
    return sl, p


# ----------------------------------------------------------------------------------------------------------------------
# autograd bridges (compat path for user code; the training loop calls the kernels directly)
# ----------------------------------------------------------------------------------------------------------------------
def _route(net, gflat, L):
    """the flat gradient of u_theta as one piece per parameter -- None for the field's (ODE_rhs) when the forward pass took no
    step (L == 1: a single time slice, at T0 or on the boundary).  The field is then no part of the function: the reference never
    puts it in the graph, its .grad stays None, and torch's Adam skips it -- no step counted, no moment decayed.  A tensor of
    zeros would count a step and, from the second sub-iteration on, move the field by its decaying moments."""
    gp = net.blob.split(gflat)
    if L == 1:
        gp = [None if n.startswith('ODE_rhs.') else g for n, g in zip(net.blob.names, gp)]
    return gp


class _OdeFn(torch.autograd.Function):
    """u_net(X).backward(): both directions are the registered operators xnwan::xnode_forward / xnode_backward (ops.py);
    this Function only routes the flat parameter gradient to the module's parameters (views of the blob)."""

    @staticmethod
    def forward(ctx, X, start, net, *params):
        blob = net.blob
        blob.check_alias()
        need = any(ctx.needs_input_grad)
        u, Y = torch.ops.xnwan.xnode_forward(X, start, blob.data, net.method, net.kdims[0], net.kdims[1], net.num_layers, need)
        ctx.net, ctx.x_dtype, ctx.s_shape, ctx.s_dtype = net, X.dtype, start.shape, start.dtype
        ctx.save_for_backward(X.detach(), start.detach(), Y)
        return u

    @staticmethod
    def backward(ctx, gu):
        net = ctx.net
        X, start, Y = ctx.saved_tensors
        want_p = any(ctx.needs_input_grad[3:])
        # The sweep always runs with its parameter part, also when every parameter is frozen: the sweep without it is another
        # kernel instantiation, whose d/dx can differ from this one's in the last bit ((20, 10, 8), rk4: one float64 ulp,
        # profiles/r22_module_surface.md) -- and the gradient X receives must not depend on which other gradients were asked for.
        # Freezing ALL of u_theta is rare on this path (the loss's helper backward passes run with the parameters live).
        gx, gs, gflat = torch.ops.xnwan.xnode_backward(gu.contiguous(), X, start, Y, net.blob.data, net.method, net.kdims[0],
                                                       net.kdims[1], net.num_layers, bool(net.adjoint), True)
        gX = None
        if ctx.needs_input_grad[0]:
            # nabla_x u is deposited at time index 0 (the model reads x from slice 0 only, src/model.py:99); the time
            # channel's gradient (non-zero only on path 0 in the reference, never read by the loss) is returned as 0
            gX = torch.zeros(X.shape, dtype=ctx.x_dtype, device=gu.device)
            gX[:, 0, 1:] = gx.to(ctx.x_dtype)
        gS = gs.view(ctx.s_shape).to(ctx.s_dtype) if ctx.needs_input_grad[1] else None
        gp = _route(net, gflat, X.shape[1]) if want_p else [None] * len(net.blob.params)
        return (gX, gS, None) + tuple(gp)


class _Dopri5Fn(torch.autograd.Function):
    """u_net(X).backward() with solver 'dopri5' (kernels.dopri5_fwd / dopri5_sweep).  A plain autograd Function, not a
    torch.library operator like _OdeFn: what the backward pass reverses is the step record of the forward pass, whose size
    (the accepted steps) is known only once the forward pass has run -- no fake kernel can state it -- so the record rides on
    ctx.  Step sizes are constants of the backward pass."""

    @staticmethod
    def forward(ctx, X, start, net, *params):
        blob = net.blob
        blob.check_alias()
        xT = X[:, 0, 1:].detach().to(F64).t().contiguous()
        t = X[0, :, 0].detach().to(F64).contiguous()
        s = start.detach().to(F64).reshape(-1).contiguous()
        N, L = X.shape[0], X.shape[1]
        u = torch.empty(L, N, dtype=F64, device=X.device)
        rec, = KN.dopri5_fwd([dict(xT=xT, start=s, u=u)], t, blob.data, net.kdims[0], net.kdims[1], net.num_layers,
                             net.hidden_dim, rtol=net.rtol, atol=net.atol, chunk=net.dopri5_chunk, max_steps=net.dopri5_max_steps,
                             stepper=net.dopri5_stepper)
        net.last_dopri5 = rec
        ctx.net, ctx.rec, ctx.x_dtype, ctx.s_shape, ctx.s_dtype = net, rec, X.dtype, start.shape, start.dtype
        ctx.save_for_backward(xT, t, s)
        return u.t().unsqueeze(2).contiguous()

    @staticmethod
    def backward(ctx, gu):
        net = ctx.net
        xT, t, s = ctx.saved_tensors
        (d, N), (H, K) = xT.shape, net.kdims
        want_p = any(ctx.needs_input_grad[3:])
        gx = torch.empty(d, N, dtype=F64, device=gu.device)
        gs = torch.empty(N, dtype=F64, device=gu.device)
        gslab = torch.empty(KN.ode_bwd_slabs(N), KN.theta_size(d, H, K), dtype=F64, device=gu.device) if want_p else None
        ubar = gu.squeeze(2).t().contiguous().to(F64)
        KN.dopri5_sweep([dict(xT=xT, start=s, ubar=ubar, gx=gx, gs=gs, gslab=gslab, rec=ctx.rec)], t, net.blob.data, H, K,
                        net.num_layers, want_x=True, want_params=want_p, stepper=net.dopri5_stepper)
        gX = None
        if ctx.needs_input_grad[0]:
            gX = torch.zeros((N, t.shape[0], d + 1), dtype=ctx.x_dtype, device=gu.device)
            gX[:, 0, 1:] = gx.t().to(ctx.x_dtype)
        gS = gs.view(ctx.s_shape).to(ctx.s_dtype) if ctx.needs_input_grad[1] else None
        gp = _route(net, KN.slab_sum(gslab), t.shape[0]) if want_p else [None] * len(net.blob.params)
        return (gX, gS, None) + tuple(gp)


class _DiscFn(torch.autograd.Function):
    """v_net(XV).backward() through xnwan::testnet_forward / testnet_backward (ops.py)"""

    @staticmethod
    def forward(ctx, XV, net, *params):
        net.blob.check_alias()
        ctx.net, ctx.dtype = net, XV.dtype
        ctx.save_for_backward(XV.detach())
        return torch.ops.xnwan.testnet_forward(XV, net.blob.data, net.kwidth, net.num_layers)

    @staticmethod
    def backward(ctx, gv):
        net = ctx.net
        XV, = ctx.saved_tensors
        want_p = any(ctx.needs_input_grad[2:])
        gX, gflat = torch.ops.xnwan.testnet_backward(gv.contiguous(), XV, net.blob.data, net.kwidth, net.num_layers,
                                                     bool(ctx.needs_input_grad[0]), want_p)
        gp = net.blob.split(gflat) if want_p else [None] * len(net.blob.params)
        return (gX.to(ctx.dtype) if ctx.needs_input_grad[0] else None, None) + tuple(gp)


# ----------------------------------------------------------------------------------------------------------------------
# modules
# ----------------------------------------------------------------------------------------------------------------------
class _EvalFn(torch.autograd.Function):
    """XNODE.evaluate_fn: u at scattered points attached to the graph of the module's parameters.  Forward is evaluate(), backward
    is evaluate_vjp() with the incoming cotangent as the weights -- it runs the checkpointing forward again, chunk by chunk."""

    @staticmethod
    def forward(ctx, points, net, n_sub, chunk, *params):
        ctx.net, ctx.n_sub, ctx.chunk = net, n_sub, chunk
        ctx.save_for_backward(points)
        return net.evaluate(points, n_sub, chunk=chunk)

    @staticmethod
    def backward(ctx, gu):
        points, = ctx.saved_tensors
        r = ctx.net.evaluate_vjp(points, gu, ctx.n_sub, ctx.chunk)
        return (None, None, None, None) + tuple(r['params'][n] for n in ctx.net.blob.names)


class _EvalGradFn(torch.autograd.Function):
    """XNODE.evaluate_grad_fn: u, du/dx and ut at scattered points attached to the graph of the module's parameters.  Forward is
    evaluate_grad(), backward is evaluate_grad_vjp() with the incoming cotangents as the weights -- it runs the checkpointing
    forward again, chunk by chunk.  A cotangent that is missing or all zero becomes None (its term is not swept)."""

    @staticmethod
    def forward(ctx, points, net, n_sub, chunk, *params):
        ctx.net, ctx.n_sub, ctx.chunk = net, n_sub, chunk
        ctx.save_for_backward(points)
        ctx.set_materialize_grads(False)
        r = net.evaluate_grad(points, n_sub, chunk)
        return r['u'], r['grad'], r['ut']

    @staticmethod
    def backward(ctx, gu, gg, gt):
        points, = ctx.saved_tensors
        gu, gg, gt = (None if g is None or not bool((g != 0).any()) else g for g in (gu, gg, gt))
        if gu is None and gg is None and gt is None:
            return (None, None, None, None) + tuple(torch.zeros_like(p) for p in ctx.net.blob.params)
        r = ctx.net.evaluate_grad_vjp(points, gu, gg, gt, ctx.n_sub, ctx.chunk)
        return (None, None, None, None) + tuple(r['params'][n] for n in ctx.net.blob.names)


class HiddenField(nn.Module):
    """dh/dt = F([x, t, h]): Linear(H+d+1, K) -> (ReLU -> tied Linear(K, K)) x (layers-1) -> Tanh -> Linear(K, H)."""

    def __init__(self, input_dim, setup, num_layers, hidden_dim):
        super().__init__()
        self.input_dim, self.hidden_dim, self.num_layers = input_dim, hidden_dim, num_layers
        if num_layers < 1:
            raise XnwanError('u_layers must be >= 1 (u_layers = 0 is the reference\'s degenerate Linear(H, H-1) field, src/model.py:138)')
        # (u_layers = 1: a field without the tied hidden layer, src/model.py:130; its slot in the blob stays zero)
        tied = [nn.ReLU(), nn.Linear(hidden_dim, hidden_dim)] * (num_layers - 1) if num_layers > 1 else []
        self.net = nn.Sequential(nn.Linear(input_dim + setup['dim'] + 1, hidden_dim), *tied, nn.Tanh(),
                                 nn.Linear(hidden_dim, input_dim)).double()

    def forward(self, h):
        raise XnwanError('the field is only evaluated inside the fused HIP stepper (XNODE.forward)')


ADAMS_ADJOINT_REFUSED = ("solver 'explicit_adams' with adjoint=True is not served: explicit_adams runs on the tiled stepper family "
                         "only, whose sweep reverses the steps taken (the discrete adjoint, step sizes as constants); torchdiffeq's "
                         "continuous adjoint exists for the fixed-grid schemes on the MFMA containers")


class XNODE(nn.Module):
    """u_theta.  forward(inputs[N, L, d+1]) -> [N, L, 1] for a group of equal-length paths (time in channel 0)."""

    def __init__(self, hidden_dim, output_dim, func_h, func_g, setup, hidden_hidden_dim, num_layers, domain,
                 solver='midpoint', min_steps=5, adjoint=False):
        super().__init__()
        if output_dim != 1:
            raise XnwanError('the PDE solution is scalar: output_dim must be 1')
        self.hidden_dim, self.output_dim, self.hidden_hidden_dim = hidden_dim, output_dim, hidden_hidden_dim
        self.h, self.g, self.setup, self.num_layers, self.domain = func_h, func_g, setup, num_layers, domain
        self.solver, self.min_steps, self.adjoint = solver, min_steps, adjoint
        self.method = KN.method_id(solver)
        if self.method == KN.DOPRI5 and adjoint:
            raise XnwanError("solver 'dopri5' with adjoint=True is not served: the sweep reverses the accepted steps (the "
                             "discrete adjoint, step sizes as constants); torchdiffeq's continuous adjoint of an adaptive solve is not built")
        if self.method == KN.ADAMS and adjoint:
            raise XnwanError(ADAMS_ADJOINT_REFUSED)
        self.rtol, self.atol = KN.DOPRI5_RTOL, KN.DOPRI5_ATOL        # (dopri5: torchdiffeq's defaults, as the reference gets them)
        self.dopri5_chunk, self.dopri5_max_steps = KN.DOPRI5_CHUNK, KN.DOPRI5_MAX_STEPS
        self.dopri5_stepper = 'vector'                               # (or 'tiled': kernels.DOPRI5_STEPPERS, EngineOptions.dopri5_stepper)
        self._ode_fn = _Dopri5Fn if self.method == KN.DOPRI5 else _OdeFn
        self.initial_layers = nn.Sequential(nn.Linear(1, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, hidden_dim),
                                            nn.ReLU(), nn.Linear(hidden_dim, hidden_dim)).double()
        self.ODE_rhs = HiddenField(hidden_dim, setup, num_layers, hidden_hidden_dim)
        self.ODE_rhs.apply(init_weights)
        self.final_linear = nn.Linear(hidden_dim, output_dim).double()
        self.blob = None

    def bind(self, device):
        """move to the device and alias the parameters to the kernels' blob, at the width of the smallest stepper
        instantiation that holds this network (kernels.ode_container; equal widths: plain concatenation) -- or at its own widths on
        the generic and tiled stepper families (kernels.stepper_family)"""
        self.to(device)
        H, K, d = self.hidden_dim, self.hidden_hidden_dim, self.setup['dim']
        self.family = KN.stepper_family(H, K, self.num_layers, method=self.method)
        if self.family == 'tiled' and self.method == KN.DOPRI5 and KN.dopri5_stepper(self.dopri5_stepper) != 'tiled':
            raise XnwanError("solver 'dopri5' runs on the generic path's field code, up to u_hidden_dim %d / u_hidden_hidden_dim %d / "
                             "u_layers %d; u_hidden_dim = %d, u_hidden_hidden_dim = %d, u_layers = %d need the tiled stepper family, "
                             "which runs the fixed-grid solvers %s only -- unless dopri5_stepper = 'tiled' (XNODE.dopri5_stepper, "
                             "EngineOptions.dopri5_stepper, XW_DOPRI5_STEPPER) selects dopri5's implementation on that family"
                             % (KN.GENERIC_ODE_MAX + (KN.GENERIC_ODE_MAX_DEPTH, H, K, self.num_layers, sorted(KN.METHODS))))
        # (the tiled family: the network's own widths, the generic layout)
        self.kdims = KN.stepper_kdims(H, K, self.num_layers, method=self.method)
        slots, total = _u_slots(d, H, K, self.kdims[0], self.kdims[1], self.num_layers > 1)
        assert total == KN.theta_size(d, *self.kdims)
        self.blob = Blob(self, device, slots, total)
        return self.blob

    def start_values(self, inputs, starts_at_T0=None):
        """h(x) for groups that start at T0, g(t0, x) for groups that start on the boundary (src/model.py:95-96);
        evaluated on the device `inputs` lives on (host tensors -> bitwise the reference's CPU values)."""
        first = inputs[:, 0, :]
        if starts_at_T0 is None:
            starts_at_T0 = float(inputs[0, 0, 0].detach()) == self.setup['T0']
        if starts_at_T0:
            return self.h(first).reshape(-1).double()
        return self.g(first.unsqueeze(1)).reshape(-1).double()

    def evaluate(self, points, n_sub=None, chunk=None, max_steps=None):
        """u_theta at scattered space-time points [M, 1 + d] (time first; host or device) -> u [M] on the network's device: every
        point is integrated from its own entry (the domain class's `entry` rule: T0 with h, or the moving boundary with g) over
        n = max(1, ceil((t - t_in) / ((T - T0) / n_sub))) equal steps ending exactly at t, n_sub = setup['N_t'] by default --
        one launch chain for the whole cloud (evalpaths.evaluate_points).  Solver 'dopri5': every point is one adaptive solve from
        its entry to t with a step controller of its own (rtol, atol of this module, the RMS norms over u_hidden_dim entries: one
        odeint call of the reference per point); n_sub must be None; max_steps: accepted steps per point (self.dopri5_max_steps),
        a point that does not get there raises.  At the blob's widths whichever stepper trains.  No gradients.  Refused: t < t_in,
        the solver 'explicit_adams', a domain class without `entry`.  chunk: paths per launch (evalpaths.EVAL_CHUNK_PATHS)."""
        from . import evalpaths
        if self.blob is None:
            raise XnwanError('XNODE.bind(device) has not been called')
        self.blob.check_alias()
        dev = self.blob.data.device
        adaptive = dict(tol=(self.rtol, self.atol), Hn=self.hidden_dim,
                        max_steps=self.dopri5_max_steps if max_steps is None else max_steps) if self.method == KN.DOPRI5 else {}
        with torch.cuda.device(dev):
            return evalpaths.evaluate_points(points, n_sub, self.setup, self.domain, self.solver, self.h, self.g, self.blob.data,
                                             self.method, self.kdims[0], self.kdims[1], self.num_layers, dev,
                                             chunk=evalpaths.EVAL_CHUNK_PATHS if chunk is None else chunk, **adaptive)

    def evaluate_grad(self, points, n_sub=None, chunk=None):
        """u_theta, its gradient in x and its time derivative at scattered space-time points [M, 1 + d] (time first; host or
        device) -> dict(u [M], grad [M, d], ut [M]) on the network's device, in one launch chain per chunk
        (evalpaths.evaluate_points_grad): evaluate()'s grids, the forward with its checkpoints kept, the reverse sweep over them.
        u: the bits of evaluate().  grad: du/dx of the discrete solution, every point's grid held fixed, the chain rule through the
        start value h([T0, x]) included (h is differentiated by autograd and taken to act point by point).  ut: FL_w . F(t, x, y(t)),
        the time derivative of the CONTINUOUS model at fixed x -- not the derivative of the discrete u with respect to the end time
        of its grid.  Solver 'dopri5': every point is one adaptive solve of its own, as in evaluate() (rtol, atol and
        dopri5_max_steps of this module; n_sub must be None), run twice -- once for u and the step counts, once with a record and
        checkpoints of exactly that size -- and grad is the reverse of every point's own accepted steps, step sizes held fixed, the
        last step through its dense output at t (training's convention for dopri5).  Refused: the solver 'explicit_adams', a
        domain class without `entry`, t < t_in, and points that are not entered at T0 (the hourglass's re-entered points: their
        entry time depends on x).  chunk: paths per launch (evalpaths.EVAL_CHUNK_PATHS, bounded further by the checkpoints'
        memory, evalpaths.EVAL_GRAD_CKPT_BYTES)."""
        return self._evaluate_grad(points, n_sub, chunk, None)

    def _evaluate_grad(self, points, n_sub, chunk, max_steps):
        """evaluate_grad with dopri5's step limit given (NODE_WAN_solver passes its option; None: self.dopri5_max_steps)"""
        from . import evalpaths
        if self.blob is None:
            raise XnwanError('XNODE.bind(device) has not been called')
        self.blob.check_alias()
        dev = self.blob.data.device
        adaptive = dict(tol=(self.rtol, self.atol), Hn=self.hidden_dim,
                        max_steps=self.dopri5_max_steps if max_steps is None else max_steps) if self.method == KN.DOPRI5 else {}
        with torch.cuda.device(dev):
            return evalpaths.evaluate_points_grad(points, n_sub, self.setup, self.domain, self.solver, self.h, self.blob.data,
                                                  self.method, self.kdims[0], self.kdims[1], self.num_layers, dev,
                                                  chunk=evalpaths.EVAL_CHUNK_PATHS if chunk is None else chunk, **adaptive)

    def evaluate_hvp(self, points, v, n_sub=None, chunk=None):
        """u_theta, its gradient in x and its Hessian in x applied to a direction per point, at scattered space-time points
        [M, 1 + d] (time first; host or device) with v [M, d] -> dict(u [M], grad [M, d], dv [M], hvp [M, d]) on the network's
        device (evalpaths.evaluate_points_hvp): evaluate_grad()'s grids and launches, then the tangent of its reverse sweep along
        (v, dh/dx . v) over the same checkpoints.  u, grad: the bits of evaluate_grad().  dv = grad . v.  hvp: the derivative of
        grad along v -- of the discrete solution x -> U(x, h([T0, x])), every point's grid held fixed, the chain rule through the
        start value to second order (h is differentiated twice by autograd and taken to act point by point), ReLU kinks as
        autograd takes them.  Time is not perturbed.  Refused: the solvers 'dopri5' and 'explicit_adams', a domain class without
        `entry`, t < t_in, points that are not entered at T0, a v of another shape.  chunk: paths per launch
        (evalpaths.EVAL_CHUNK_PATHS, bounded further by the memory of the checkpoints and their tangents)."""
        return self._evaluate_second('evaluate_points_hvp', (points, v, n_sub), chunk)

    def evaluate_hess(self, points, n_sub=None, chunk=None):
        """u_theta, its gradient, its Hessian in x and its Laplacian at scattered space-time points [M, 1 + d] ->
        dict(u [M], grad [M, d], hess [M, d, d], lap [M]) on the network's device (evalpaths.evaluate_points_hess): evaluate_hvp()'s
        chain with the d unit directions, the forward and the gradient sweep once per chunk; row k of hess is the product with
        e_k.  hess is not symmetrised (its asymmetry is rounding); lap is its trace.  Refusals: evaluate_hvp()'s."""
        return self._evaluate_second('evaluate_points_hess', (points, n_sub), chunk)

    def evaluate_quad(self, points, V, n_sub=None, chunk=None):
        """u_theta and its first and second directional derivatives in x along R directions per point, at scattered space-time
        points [M, 1 + d] (time first; host or device) with V [M, R, d] -> dict(u [M], dv [M, R], quad [M, R]) on the network's
        device (evalpaths.evaluate_points_quad): ONE launch per chunk, a second-order forward jet along every point's own grid --
        no reverse sweep, no checkpoints.  u: the bits of evaluate().  dv = grad . v_r.  quad = v_r^T (d^2u/dx^2) v_r of the
        discrete solution x -> U(x, h([T0, x])), every point's grid held fixed, the chain rule through the start value to second
        order, ReLU kinks as autograd takes them.  Time is not perturbed.  Refusals: evaluate_hvp()'s, and a V of another shape.
        chunk: paths per launch (evalpaths.EVAL_CHUNK_PATHS, bounded further by the workspace's memory, a block per tile and
        direction)."""
        return self._evaluate_second('evaluate_points_quad', (points, V, n_sub), chunk)

    def evaluate_lap(self, points, a=None, n_sub=None, chunk=None):
        """u_theta and the diffusion term sum_ij a_ij d^2u/dx_i dx_j at scattered space-time points [M, 1 + d] ->
        dict(u [M], lap [M]) on the network's device (evalpaths.evaluate_points_lap): evaluate_quad()'s launch with d directions --
        a None: the Laplacian; a [d, d] or [M, d, d]: the unit directions weighted by a_kk where a is diagonal, else the
        eigenvectors and eigenvalues of its symmetric part.  Derivatives of the discrete solution, every point's grid held fixed;
        evaluate_hess()'s `lap` without the [M, d, d] output.  Refusals: evaluate_quad()'s, and an `a` of another shape."""
        return self._evaluate_second('evaluate_points_lap', (points, a, n_sub), chunk)

    def evaluate_vjp(self, points, w, n_sub=None, chunk=None):
        """u_theta at scattered space-time points [M, 1 + d] (time first; host or device) and the weighted sum of its PARAMETER
        gradients, with a weight per point w [M] -> dict(u [M], params {name: tensor}, start [M]) on the network's device
        (evalpaths.evaluate_points_vjp): evaluate_grad()'s grids and forward with its checkpoints kept, then a reverse sweep that
        writes parameter gradients, chunk by chunk.  u: the bits of evaluate().  params: sum_p w_p dU_p/dtheta, one tensor per
        parameter of this module under its named_parameters() name and in its shape -- U_p the discrete solution at point p, every
        point's grid and step sizes held fixed, the start value h([T0, x]) a constant of theta, ReLU kinks as autograd takes them:
        what autograd gives for sum_p w_p u_p through the fixed-grid odeint, every point on a path of its own.  start: w_p
        dU_p/dstart_p, what reaches the start values (h is not differentiated).
        Where no point takes a step (every t == T0) the field's (ODE_rhs) entries are tensors of ZEROS, not None.  That differs
        from forward().backward() on a single time slice, which leaves the field's .grad at None because the reference never puts
        the field in the graph there and an optimiser must see the same; here there is no reference call to follow -- a cloud
        mixes points with and without steps, the field is part of the function, and its gradient at such a cloud is zero.
        Refused: the solvers 'dopri5' and 'explicit_adams', a domain class without `entry`, t < t_in, points that are not entered
        at T0, a w of another shape.  chunk: paths per launch (evalpaths.EVAL_CHUNK_PATHS, bounded further by the memory of the
        checkpoints and the slabs, evalpaths.vjp_chunk_paths)."""
        r = self._evaluate_second('evaluate_points_vjp', (points, w, n_sub), chunk)
        return dict(u=r['u'], params=dict(zip(self.blob.names, self.blob.split(r['gflat']))), start=r['start'])

    def evaluate_fn(self, points, n_sub=None, chunk=None):
        """evaluate() attached to the autograd graph of this module's parameters: u [M] on the network's device, so that
        ((net.evaluate_fn(points) - data) ** 2).mean().backward() and any torch optimiser on the parameters work -- a
        torch.autograd.Function whose forward is evaluate() and whose backward is evaluate_vjp() with the incoming cotangent as the
        weights (the gradient of the discrete solution, every point's grid held fixed, the start value a constant of theta).  The
        backward runs the forward again with its checkpoints kept.  No gradient reaches `points`: points that require grad are
        refused -- evaluate_grad() gives du/dx.  Refusals otherwise: evaluate_vjp()'s."""
        if self.blob is None:
            raise XnwanError('XNODE.bind(device) has not been called')
        if torch.is_tensor(points) and points.requires_grad:
            raise XnwanError('evaluate_fn(): points that require grad are not served -- the function is attached to the parameters\' '
                             'graph only; evaluate_grad() gives du/dx at scattered points')
        from . import evalpaths
        evalpaths.vjp_refuse_solver(self.solver)                 # (before the forward runs: evaluate() serves dopri5, the backward would not)
        return _EvalFn.apply(points, self, n_sub, chunk, *self.blob.params)

    def evaluate_grad_vjp(self, points, wu=None, wg=None, wt=None, n_sub=None, chunk=None):
        """u_theta, its gradient in x and its time derivative at scattered space-time points [M, 1 + d] (time first; host or
        device) and the PARAMETER gradient of their weighted sum, with weights wu [M], wg [M, d], wt [M] (each may be None: zeros;
        not all three) -> dict(u [M], grad [M, d], ut [M], params {name: tensor}) on the network's device
        (evalpaths.evaluate_points_grad_vjp): evaluate_grad()'s launches, then the tangent of evaluate_vjp()'s sweep along
        (wg, dh/dx . wg), chunk by chunk.  u, grad, ut: the bits of evaluate_grad().  params: d/dtheta sum_p [wu_p u_p + wg_p .
        grad_p + wt_p ut_p] in evaluate_vjp()'s layout and names -- of the discrete solution, every point's grid and step sizes held
        fixed, the start value h([T0, x]) and its gradient dh/dx constants of theta, ReLU kinks as autograd takes them: what
        autograd gives for that sum with create_graph on the x-gradient, every point on a path of its own.  ut is the CONTINUOUS
        model's time derivative FL_w . F(t, x, y(t)); theta enters it through the read-out, the field and y(t).  The field's
        entries are tensors of zeros, not None, where nothing reaches them (evaluate_vjp() says why).
        Refused: the solvers 'dopri5' and 'explicit_adams', a domain class without `entry`, t < t_in, points that are not entered
        at T0, all three weights None, a weight of another shape.  chunk: paths per launch (evalpaths.EVAL_CHUNK_PATHS, bounded
        further by the memory of both sets of checkpoints and the slabs, evalpaths.gvjp_chunk_paths)."""
        r = self._evaluate_second('evaluate_points_grad_vjp', (points, wu, wg, wt, n_sub), chunk)
        return dict(u=r['u'], grad=r['grad'], ut=r['ut'], params=dict(zip(self.blob.names, self.blob.split(r['gflat']))))

    def evaluate_grad_fn(self, points, n_sub=None, chunk=None):
        """evaluate_grad() attached to the autograd graph of this module's parameters: dict(u [M], grad [M, d], ut [M]) on the
        network's device, so that a first-order strong-form residual or a flux fit trains --
            r = net.evaluate_grad_fn(pts)
            loss = ((r['ut'] + (B * r['grad']).sum(1) + c * r['u'] - f) ** 2).mean() + ((r['grad'] - flux) ** 2).mean()
            loss.backward(); opt.step()
        -- ONE torch.autograd.Function with three outputs whose forward is evaluate_grad() and whose backward is
        evaluate_grad_vjp() with the incoming cotangents as the weights (a missing or all-zero cotangent: None).  The backward
        runs the forward again with its checkpoints kept.  What is held fixed is evaluate_grad_vjp()'s: grids, step sizes, h and
        dh/dx.  No gradient reaches `points`, and no second derivative in theta is built (the outputs' graph ends at this
        Function): points that require grad are refused.  Refusals otherwise: evaluate_grad_vjp()'s."""
        if self.blob is None:
            raise XnwanError('XNODE.bind(device) has not been called')
        if torch.is_tensor(points) and points.requires_grad:
            raise XnwanError('evaluate_grad_fn(): points that require grad are not served -- the function is attached to the '
                             'parameters\' graph only; evaluate_hvp() gives the derivative of du/dx in x')
        from . import evalpaths
        evalpaths.grad_vjp_refuse_solver(self.solver)            # (before the forward runs: evaluate_grad() serves dopri5, the backward would not)
        u, grad, ut = _EvalGradFn.apply(points, self, n_sub, chunk, *self.blob.params)
        return dict(u=u, grad=grad, ut=ut)

    def _evaluate_second(self, name, args, chunk, **kw):
        from . import evalpaths
        if self.blob is None:
            raise XnwanError('XNODE.bind(device) has not been called')
        self.blob.check_alias()
        dev = self.blob.data.device
        with torch.cuda.device(dev):
            return getattr(evalpaths, name)(*args, self.setup, self.domain, self.solver, self.h, self.blob.data, self.method,
                                            self.kdims[0], self.kdims[1], self.num_layers, dev,
                                            chunk=evalpaths.EVAL_CHUNK_PATHS if chunk is None else chunk, **kw)

    def forward(self, inputs, starts_at_T0=None):
        """starts_at_T0 (optional): the caller knows where the paths start -- True: at T0 (start values h), False: on the
        moving boundary (start values g; the sampler's late-entry groups).  Saves reading inputs[0, 0, 0] / max(w) back from the
        device, which waits for everything queued on it (the training loop's diagnostic passes it).  None: looked up, and
        paths that start neither at T0 nor on the boundary take the evaluation path (bound_pad)."""
        if self.blob is None:
            raise XnwanError('XNODE.bind(device) has not been called')
        served = self.__dict__.get('_served')
        if served is not None and inputs is served[0] and not torch.is_grad_enabled():
            # the training loop's own sample, asked for by a `stop` hook (solver._stop_agreed): the group's device buffers already
            # hold the points, the grid and the start values -- the stepper's forward kernel is launched on them directly
            return served[1]()
        dev = self.blob.data.device
        known = starts_at_T0 is not None
        if starts_at_T0 is None:
            starts_at_T0 = float(inputs[0, 0, 0].detach()) == self.setup['T0']
        gather = None
        if not starts_at_T0 and not known:
            on_boundary = float(torch.max(self.domain.func_w(inputs[:, 0, :].detach().unsqueeze(1)))) < 1e-5
            if not on_boundary:
                if self.method == KN.DOPRI5:
                    raise XnwanError("solver 'dopri5': paths that start neither at T0 nor on the boundary (the evaluation path over "
                                     "domain.bound_pad's densified grids) are not served")
                # evaluation of points that are neither at T0 nor on the boundary (src/model.py:92-106): integrate from T0
                # over the densified grid of domain.bound_pad / fillt and keep the states at the requested times
                path_i, gather, filled = self.domain.bound_pad(inputs.detach())
                if path_i is not None:
                    # per-bucket grids (hourglass): like the reference, ALL paths are integrated over the bucket's grid
                    # and the bucket's rows / columns are kept; the result is ordered bucket by bucket (src/model.py:104-109)
                    start = self.start_values(inputs)
                    outs = []
                    for rows, cols, grid in zip(path_i, gather, filled):
                        grid = grid.to(inputs.device).to(inputs.dtype).reshape(-1)
                        padded = inputs[:, :1, :].repeat(1, grid.shape[0], 1)
                        padded[:, :, 0] = grid.view(1, -1)
                        out = self._ode_fn.apply(padded.to(dev), start.to(dev), self, *self.blob.params)
                        outs.append(out[rows.to(dev)][:, cols.long().to(dev), :])
                    return torch.cat(outs, dim=0)
                grid = filled.to(inputs.device).to(inputs.dtype)
                padded = inputs[:, :1, :].repeat(1, grid.shape[0], 1)
                padded[:, :, 0] = grid.view(1, -1)
                start = self.start_values(inputs)
                out = self._ode_fn.apply(padded.to(dev), start.to(dev), self, *self.blob.params)
                return out[:, gather.long().to(dev), :]
        out = self._ode_fn.apply(inputs.to(dev), self.start_values(inputs, starts_at_T0).to(dev), self, *self.blob.params)
        if inputs.shape[1] == 1 and starts_at_T0:
            return out[:, 0, :]                                   # reference returns [N, 1] here (src/model.py:89-91)
        return out


class TestNet(nn.Module):
    """v_phi: Linear(d+1, W) -> (ReLU -> tied Linear(W, W)) x v_layers -> Tanh -> Linear(W, 1), pointwise on [..., d+1]."""
    __test__ = False

    def __init__(self, config, setup):
        super().__init__()
        self.num_layers, self.hidden_dim = config['v_layers'], config['v_hidden_dim']
        self.input = nn.Linear(setup['dim'] + 1, self.hidden_dim)
        self.hidden = nn.Linear(self.hidden_dim, self.hidden_dim)
        self.output = nn.Linear(self.hidden_dim, 1)
        self.net = nn.Sequential(self.input, *[nn.ReLU(), self.hidden] * self.num_layers, nn.Tanh(), self.output)
        self.net.double()
        self.blob = None

    def bind(self, device):
        self.to(device)
        d = self.input.in_features - 1
        # the family (kernels.testnet_family): the MFMA containers / generic path at the container's width, or the tiled
        # family at the network's own width
        self.family = KN.testnet_family(self.hidden_dim, self.num_layers)
        self.kwidth = KN.testnet_kwidth(self.hidden_dim, self.num_layers)
        slots, total = _v_slots(d, self.hidden_dim, self.kwidth)
        assert total == KN.phi_size(d, self.kwidth)
        self.blob = Blob(self, device, slots, total)
        return self.blob

    def forward(self, XV):
        if self.blob is None:
            raise XnwanError('TestNet.bind(device) has not been called')
        return _DiscFn.apply(XV.to(self.blob.data.device), self, *self.blob.params)


class PathParallel(nn.Module):
    """Stands where the reference has nn.DataParallel: same `.module` attribute and `module.` state_dict prefix.
    Monte-Carlo paths are sharded across GPUs by one process per GPU (dist.py), not by this wrapper."""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, *a, **kw):
        return self.module(*a, **kw)


# names under which the reference exports these classes (src/model.py)
NeuralODE = XNODE
discriminator = TestNet
_ODEField = HiddenField
