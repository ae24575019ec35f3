"""u_theta at scattered space-time points: every point is the end of a path of its own, on a time grid of its own.

The stepper entry points take ONE grid t[L] for all paths of a job; kernels.tiled_paths_fwd (csrc/xw_tiled_paths.hip) takes a
grid per path.  This module is the host side of it: the per-point grids (step_counts, pack_grids), the sort that makes the 16-path
tiles homogeneous in their step count (sort_by_steps), the chunked launch (paths_forward) and the evaluation itself
(evaluate_points, behind XNODE.evaluate / NODE_WAN_solver.evaluate).

A point (t, x) is entered at (t_in, x) -- the domain class's `entry` rule: T0 with the start value h, or the moving boundary
with g -- and integrated over n = max(1, ceil((t - t_in) / ((T - T0) / n_sub))) equal steps that end exactly at t; t == t_in takes
none.  No gradients, no collective calls, no random numbers.

Solver 'dopri5' has no grid to pack: kernels.paths_dopri5_fwd (csrc/xw_tdopri_paths.hip) runs a step controller per path from
t_in to t -- one odeint call of the reference per point -- and paths_dopri5 chunks it, with one read-back of the status words per
chunk; evaluate_points takes it with tol = (rtol, atol).

Gradients come from evaluate_points_grad alone (behind XNODE.evaluate_grad / NODE_WAN_solver.evaluate_grad): the fixed-grid forward
with its checkpoints kept, then kernels.tiled_paths_grad (csrc/xw_tiled_paths_grad.hip), the reverse sweep over the same ragged
group, and the chain rule through the start value (start_gradient).  Its docstring says what its `ut` is and what it refuses.
With solver 'dopri5' (tol given) it is three passes: paths_dopri5 for u and every path's step count, then, sorted by that count and
cut by dopri5_grad_chunks, the same forward with its record and checkpoints kept and kernels.paths_dopri5_grad
(csrc/xw_tdopri_paths_grad.hip), the reverse sweep over every path's own accepted steps (dopri5_grad_pass).

Second derivatives come from evaluate_points_hvp and evaluate_points_hess (behind evaluate_hvp / evaluate_hess of XNODE and
NODE_WAN_solver), for the fixed-grid schemes: the forward and the gradient sweep as above, then kernels.tiled_paths_hvp
(csrc/xw_tiled_paths_hvp.hip), the tangent of that sweep along a direction per point, once per direction over the same checkpoints,
and the chain rule through the start value to second order (start_gradient, start_hvp).

Quadratic forms of the Hessian, the diffusion term sum a_ij d_ij u and the strong-form residual come from evaluate_points_quad,
evaluate_points_lap and evaluate_points_residual (behind evaluate_quad / evaluate_lap of XNODE and NODE_WAN_solver and
NODE_WAN_solver.evaluate_residual): kernels.tiled_paths_jet (csrc/xw_tiled_paths_jet.hip), a second-order forward jet along every
point's own grid, R directions per point in one launch per chunk -- no reverse sweep, no checkpoints, no [M, d, d] output.

Parameter gradients come from evaluate_points_vjp (behind XNODE.evaluate_vjp / evaluate_fn and NODE_WAN_solver.evaluate_vjp), for
the fixed-grid schemes: the forward with its checkpoints kept, then kernels.tiled_paths_vjp (csrc/xw_tiled_paths_vjp.hip), the
gradient sweep with a weight per point that writes a slab per tile, and kernels.slab_sum into one flat gradient, chunk by chunk.

Parameter gradients of du/dx and ut as well come from evaluate_points_grad_vjp (behind XNODE.evaluate_grad_vjp / evaluate_grad_fn
and NODE_WAN_solver.evaluate_grad_vjp): the forward, the gradient sweep and the tangent forward of kernels.tiled_paths_hvp, then
kernels.tiled_paths_gvjp (csrc/xw_tiled_paths_gvjp.hip), the tangent of the slab-writing sweep along (wg, dh/dx . wg) with the
weights on u and ut folded into its start."""
import types

import torch

from . import kernels as KN
from ._lib import XnwanError

F64 = torch.float64
EVAL_CHUNK_PATHS = 65536                   # EngineOptions.eval_chunk_paths
REFUSED_SOLVERS = ('dopri5', 'explicit_adams')
EVAL_GRAD_CKPT_BYTES = 1 << 30             # evaluate_points_grad: a chunk's checkpoints (Y [L, H, n]; dopri5: ckpt [cap, H, n]) stay below this


def step_counts(t, t_in, T0, T, n_sub):
    """steps per point, int64 [M]: 0 where t == t_in, else max(1, ceil((t - t_in) / ((T - T0) / n_sub))); t, t_in float64"""
    step = (T - T0) / n_sub
    n = torch.ceil((t - t_in) / step).clamp(min=1).to(torch.int64)
    return torch.where(t == t_in, torch.zeros_like(n), n)


def pack_grids(t, t_in, n):
    """the grids, time-major tT [max n + 1, M] float64: row l of point i is t_in + (t - t_in) l / n_i for l < n_i and t itself
    from l = n_i on (the grid ends exactly at t; the rows behind it repeat it: zero-length steps)"""
    L = int(n.max()) + 1 if n.numel() else 1
    l = torch.arange(L, dtype=F64, device=t.device).view(L, 1)
    grid = t_in.view(1, -1) + (t - t_in).view(1, -1) * l / n.clamp(min=1).to(F64).view(1, -1)
    return torch.where(l >= n.view(1, -1), t.view(1, -1).expand(L, -1), grid).contiguous()


def sort_by_steps(n):
    """(order, inverse): order sorts the points by their step count (stable), inverse[order[k]] = k puts results back"""
    order = torch.argsort(n, stable=True)
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(order.numel(), device=order.device)
    return order, inverse


def last_distinct(tT):
    """nstep [N] int32 of a packed group tT [L, N]: the index of each path's last time that differs from the one before it"""
    L = tT.shape[0]
    if L == 1:
        return torch.zeros(tT.shape[1], dtype=torch.int32, device=tT.device)
    idx = torch.arange(1, L, device=tT.device).view(L - 1, 1)
    return ((tT[1:] != tT[:-1]) * idx).amax(0).to(torch.int32)


def paths_forward(xT, tT, start, nstep, theta, method, H, K, m, last_only=False, chunk=EVAL_CHUNK_PATHS):
    """kernels.tiled_paths_fwd on N paths, at most `chunk` of them per launch (the launches share the stream and so the
    workspace's memory: it is bounded by the chunk): u [L, N], or [N] with last_only"""
    N, L = xT.shape[1], tT.shape[0]
    if chunk < 1:
        raise XnwanError('eval_chunk_paths = %d: at least one path per launch' % chunk)
    if N <= chunk:
        u = torch.empty((N,) if last_only else (L, N), dtype=F64, device=xT.device)
        KN.tiled_paths_fwd([dict(xT=xT, start=start, tT=tT, nstep=nstep, u=u)], theta, method, H, K, m, last_only=last_only)
        return u
    parts = []
    for lo in range(0, N, chunk):
        hi = min(lo + chunk, N)
        parts.append(paths_forward(xT[:, lo:hi].contiguous(), tT[:, lo:hi].contiguous(), start[lo:hi].contiguous(),
                                   None if nstep is None else nstep[lo:hi].contiguous(), theta, method, H, K, m, last_only, chunk))
    return torch.cat(parts, -1)


def paths_dopri5(xT, t_in, t_end, start, theta, H, K, m, Hn, rtol, atol, max_steps=KN.DOPRI5_MAX_STEPS, max_attempts=None,
                 chunk=EVAL_CHUNK_PATHS):
    """kernels.paths_dopri5_fwd on N paths, at most `chunk` of them per launch, ONE read-back of the status words per chunk:
    dict(u [N], fin [2, N] on the device; status, n_acc, n_att [N] int32 on the host).  Nothing is raised for a status."""
    N, dev = xT.shape[1], xT.device
    if chunk < 1:
        raise XnwanError('eval_chunk_paths = %d: at least one path per launch' % chunk)
    u = torch.empty(N, dtype=F64, device=dev)
    fin = torch.empty(2, N, dtype=F64, device=dev)
    words = torch.empty(3, N, dtype=torch.int32)
    for lo in range(0, N, chunk):
        n = min(lo + chunk, N) - lo
        whole = n == N
        w = torch.empty(3, n, dtype=torch.int32, device=dev)
        job = dict(xT=xT if whole else xT[:, lo:lo + n].contiguous(), start=start[lo:lo + n], t_in=t_in[lo:lo + n],
                   t_end=t_end[lo:lo + n], u=u[lo:lo + n], status=w[0], n_acc=w[1], n_att=w[2],
                   fin=fin if whole else torch.empty(2, n, dtype=F64, device=dev))
        KN.paths_dopri5_fwd([job], theta, H, K, m, Hn, rtol=rtol, atol=atol, max_steps=max_steps, max_attempts=max_attempts)
        if not whole:
            fin[:, lo:lo + n] = job['fin']
        words[:, lo:lo + n] = w.cpu()                        # (the chunk's one read-back: waits for its launch)
    return dict(u=u, fin=fin, status=words[0], n_acc=words[1], n_att=words[2])


def raise_unreached(who, r, order, inverse, t, t_in, max_steps):
    """XnwanError for the paths of r = paths_dopri5(...) (sorted by `order`) whose controller ended with a status: their count and
    the first such point as the caller numbers them, with dopri5_status_message's words; nothing where every status is 0"""
    bad = (r['status'] != 0).nonzero().view(-1)
    if bad.numel():
        i = int(order[bad.to(order.device)].min())
        k = int(inverse[i])
        fin = r['fin'][:, k].tolist()
        msg = KN.dopri5_status_message(int(r['status'][k]), [fin[0], fin[1], int(r['n_acc'][k]), int(r['n_att'][k])], max_steps)
        raise XnwanError('%s: %d of %d points did not reach their time (first: point %d, t = %r, t_in = %r): %s'
                         % (who, bad.numel(), t.numel(), i, float(t[i]), float(t_in[i]), msg))


def start_gradient(h, first):
    """dh/dx [M, d] at first = [t_in, x] ([M, 1 + d]): torch.autograd.grad of h(first).sum() with respect to a leaf copy of
    `first`, the time column dropped.  h is taken to act POINT BY POINT -- row i of its output depends on row i of its input alone,
    as every shipped func_h does -- so the gradient of the sum is, row by row, the gradient of each start value.  Exact zeros where
    h's output does not depend on its input (a constant h: no grad_fn, or an unused input)."""
    with torch.enable_grad():
        leaf = first.detach().clone().requires_grad_(True)
        out = h(leaf)
        if not (torch.is_tensor(out) and out.requires_grad):
            return torch.zeros_like(first[:, 1:])
        grad, = torch.autograd.grad(out.sum(), leaf, allow_unused=True)
    if grad is None:
        return torch.zeros_like(first[:, 1:])
    return grad[:, 1:].detach().to(first.dtype)


def grad_chunk_paths(chunk, L, H):
    """paths per launch of evaluate_points_grad: the checkpoints Y [L, H, n] of a chunk stay below EVAL_GRAD_CKPT_BYTES (whole
    16-path tiles, at least one) -- a memory bound, not a tuned number"""
    return min(chunk, max(16, 16 * (EVAL_GRAD_CKPT_BYTES // (8 * L * H * 16))))


def dopri5_grad_chunks(n_acc_sorted, H, chunk, budget=EVAL_GRAD_CKPT_BYTES):
    """[(lo, hi, cap)]: the launches of dopri5_grad_pass over paths sorted by their accepted step count n_acc_sorted (a sequence of
    ints).  cap = max(1, the largest count of the chunk), the slots of its record; hi - lo <= chunk; chunks are whole 16-path tiles
    (the last one, or a chunk below 16, apart); and the checkpoints 8 cap H (hi - lo) bytes stay within `budget` wherever a chunk
    holds more than one tile -- a memory bound, not a tuned number.  Every path is in exactly one chunk."""
    n = [int(v) for v in n_acc_sorted]
    if chunk < 1:
        raise XnwanError('eval_chunk_paths = %d: at least one path per launch' % chunk)
    limit = chunk - chunk % 16 if chunk >= 16 else chunk
    out, lo = [], 0
    while lo < len(n):
        hi, cap = lo, 1
        while hi < len(n) and hi - lo < limit:
            nxt = min(hi + 16, len(n), lo + limit)
            grown = max(cap, max(n[hi:nxt]))
            if hi > lo and 8 * grown * H * (nxt - lo) > budget:
                break
            hi, cap = nxt, grown
        out.append((lo, hi, cap))
        lo = hi
    return out


def dopri5_grad_pass(xT, t_in, t_end, start, n_acc, theta, H, K, m, Hn, rtol, atol, max_steps=KN.DOPRI5_MAX_STEPS,
                     chunk=EVAL_CHUNK_PATHS):
    """the second forward and the sweep of evaluate_points_grad with solver 'dopri5', on N paths whose controllers have ended with
    status 0 after n_acc [N] (host, int) accepted steps: the paths are sorted by that count (stable), so that the 16 paths of a tile
    walk about the same rounds back, cut by dopri5_grad_chunks, and per chunk kernels.paths_dopri5_fwd runs again with rec, ckpt
    and Y of exactly the chunk's largest count, then kernels.paths_dopri5_grad.  -> dict(u [N], gx [d, N], gs [N], ut [N]) on the
    device, in the caller's order; u: the second forward's, the bits of the first (a path's bits depend on neither order nor
    neighbours).  Nothing is read back."""
    (d, N), dev = xT.shape, xT.device
    order, inverse = sort_by_steps(torch.as_tensor(n_acc, dtype=torch.int64).cpu())
    od = order.to(dev)
    xs, ts, te, ss = xT[:, od].contiguous(), t_in[od].contiguous(), t_end[od].contiguous(), start[od].contiguous()
    u = torch.empty(N, dtype=F64, device=dev)
    gx = torch.empty(d, N, dtype=F64, device=dev)
    gs, ut = torch.empty(N, dtype=F64, device=dev), torch.empty(N, dtype=F64, device=dev)
    for lo, hi, cap in dopri5_grad_chunks(torch.as_tensor(n_acc)[order].tolist(), H, chunk):
        k, whole = hi - lo, hi - lo == N
        words = torch.empty(3, k, dtype=torch.int32, device=dev)
        job = dict(xT=xs if whole else xs[:, lo:hi].contiguous(), start=ss[lo:hi], t_in=ts[lo:hi], t_end=te[lo:hi], u=u[lo:hi],
                   status=words[0], n_acc=words[1], n_att=words[2], Y=torch.empty(H, k, dtype=F64, device=dev),
                   rec=torch.empty(cap, 2, k, dtype=F64, device=dev), ckpt=torch.empty(cap, H, k, dtype=F64, device=dev))
        KN.paths_dopri5_fwd([job], theta, H, K, m, Hn, rtol=rtol, atol=atol, max_steps=max_steps)
        out = dict(gx=gx if whole else torch.empty(d, k, dtype=F64, device=dev), gs=gs[lo:hi], ut=ut[lo:hi])
        KN.paths_dopri5_grad([dict(job, **out)], theta, H, K, m)
        if not whole:
            gx[:, lo:hi] = out['gx']
    inv = inverse.to(dev)
    return dict(u=u[inv], gx=gx[:, inv], gs=gs[inv], ut=ut[inv])


def evaluate_points_grad(points, n_sub, setup, domain, solver, h, theta, method, H, K, m, device, chunk=EVAL_CHUNK_PATHS, tol=None,
                         Hn=None, max_steps=KN.DOPRI5_MAX_STEPS):
    """u_theta, its gradient in x and its time derivative at points [M, 1 + d] (time first; host or device, float32 or float64)
    -> dict(u [M], grad [M, d], ut [M]), float64 on `device`.  Entry rule, step counts, packing and sort are evaluate_points';
    per chunk kernels.tiled_paths_fwd keeps the checkpoints and kernels.tiled_paths_grad walks them back:
      u     the forward's last row: the bits of evaluate_points
      grad  du/dx of the DISCRETE solution with every point's grid held fixed: gx + gs * dh/dx (start_gradient: the chain rule
            through the start value h([T0, x]))
      ut    FL_w . F(t, x, y(t)): the time derivative of the CONTINUOUS model y' = F, u = FL y at fixed x -- not the derivative
            of the discrete u with respect to the end time of its grid (that would need the derivative of the steps in dt).
    tol = (rtol, atol) with solver 'dopri5' (Hn, max_steps: as evaluate_points takes them; n_sub must be None): every point is one
    adaptive solve of its own, and the chain is three passes -- paths_dopri5 as evaluate_points runs it, for u (the bits of
    evaluate_points), the status words and every path's count of accepted steps; then dopri5_grad_pass: the same forward again,
    sorted by that count, with a record and checkpoints of exactly the size it needs, and the reverse sweep over them.  grad is
    then du/dx of the discrete solution with every point's ACCEPTED STEPS held fixed (step sizes as constants, the last step
    through its dense output at t: training's convention); ut as above, at the forward's y(t).
    Refused: the solver 'explicit_adams', 'dopri5' without tol, a domain class without `entry`, t < t_in, and every point that is
    not entered at T0 -- the hourglass's re-entered points, whose entry time |x| / r depends on x: holding it fixed would not give
    the gradient.  No collective calls, no random numbers."""
    adaptive = solver == 'dopri5' and tol is not None
    if solver in REFUSED_SOLVERS and not adaptive:
        raise XnwanError("evaluate_grad(): solver %r is not served -- the reverse sweep over per-path time grids runs the fixed-grid "
                         "schemes %s only (it reverses the steps taken; no per-path step controller or multistep history is built)"
                         % (solver, sorted(KN.METHODS)))
    if adaptive and n_sub is not None:
        raise XnwanError("evaluate_grad(): n_sub = %r with solver 'dopri5' -- every point's step sizes are its controller's (rtol, "
                         "atol); a number of steps over [T0, T] has no meaning there" % (n_sub,))
    entry = getattr(domain, 'entry', None)
    if entry is None:
        name = getattr(domain, '__name__', type(domain).__name__)
        raise XnwanError('evaluate_grad(): the domain class %s has no entry(points, shape_param, T0, T) rule: where a point\'s path '
                         'starts, and with which start value, is the domain\'s to say' % name)
    d, T0, T = setup['dim'], setup['T0'], setup['T']
    n_sub = setup['N_t'] if n_sub is None else n_sub
    if not adaptive and n_sub < 1:
        raise XnwanError('evaluate_grad(): n_sub = %r, at least one step over [T0, T]' % (n_sub,))
    if chunk < 1:
        raise XnwanError('eval_chunk_paths = %d: at least one path per launch' % chunk)
    if not (torch.is_tensor(points) and points.dim() == 2 and points.shape[1] == 1 + d):
        raise XnwanError('evaluate_grad(): points must be a tensor [M, 1 + d] = [M, %d], time first' % (1 + d))
    with torch.no_grad():
        pts = points.detach().to(F64)
        M = pts.shape[0]
        if M == 0:
            return dict(u=torch.empty(0, dtype=F64, device=device), grad=torch.empty(0, d, dtype=F64, device=device),
                        ut=torch.empty(0, dtype=F64, device=device))
        t = pts[:, 0].contiguous()
        t_in, at_T0 = entry(pts, setup['shape_param'], T0, T)
        early = t < t_in
        if bool(early.any()):
            i = int(early.nonzero()[0])
            raise XnwanError('evaluate_grad(): %d points lie before their entry time (t >= t_in is the limit; first: point %d, '
                             't = %r, t_in = %r)' % (int(early.sum()), i, float(t[i]), float(t_in[i])))
        late = ~at_T0
        if bool(late.any()):
            i = int(late.nonzero()[0])
            raise XnwanError('evaluate_grad(): %d points are not entered at T0 (entry at T0 is the limit; first: point %d, t = %r, '
                             't_in = %r): their path starts on the moving boundary at a time that depends on x, and a gradient '
                             'with that time held fixed is not du/dx' % (int(late.sum()), i, float(t[i]), float(t_in[i])))
        first = torch.cat((t_in.view(-1, 1), pts[:, 1:]), 1)
        s = h(first).reshape(-1).double()
        hx = start_gradient(h, first).to(F64)
        if adaptive:
            Hn, rtol, atol = H if Hn is None else Hn, float(tol[0]), float(tol[1])
            order, inverse = sort_by_steps(t - t_in)         # (evaluate_points' sort: by the length of the interval)
            xT, ts = pts[order, 1:].t().contiguous().to(device), t_in[order].contiguous().to(device)
            te, start = t[order].contiguous().to(device), s[order].contiguous().to(device)
            r = paths_dopri5(xT, ts, te, start, theta, H, K, m, Hn, rtol, atol, max_steps=max_steps, chunk=chunk)
            raise_unreached('evaluate_grad()', r, order, inverse, t, t_in, max_steps)
            g = dopri5_grad_pass(xT, ts, te, start, r['n_acc'], theta, H, K, m, Hn, rtol, atol, max_steps=max_steps, chunk=chunk)
            inv = inverse.to(device)
            grad = g['gx'].t()[inv] + g['gs'][inv].view(-1, 1) * hx.to(device)
            return dict(u=r['u'][inv], grad=grad.contiguous(), ut=g['ut'][inv])
        n = step_counts(t, t_in, T0, T, n_sub)
        order, inverse = sort_by_steps(n)
        tT = pack_grids(t[order], t_in[order], n[order]).to(device)
        xT = pts[order, 1:].t().contiguous().to(device)
        start, nstep = s[order].contiguous().to(device), n[order].to(torch.int32).to(device)
        L = tT.shape[0]
        per = grad_chunk_paths(chunk, L, H)
        u = torch.empty(M, dtype=F64, device=device)
        gx = torch.empty(d, M, dtype=F64, device=device)
        gs, ut = torch.empty(M, dtype=F64, device=device), torch.empty(M, dtype=F64, device=device)
        for lo in range(0, M, per):
            k = min(lo + per, M) - lo
            whole = k == M
            job = dict(xT=xT if whole else xT[:, lo:lo + k].contiguous(), start=start[lo:lo + k],
                       tT=tT if whole else tT[:, lo:lo + k].contiguous(), nstep=nstep[lo:lo + k],
                       u=torch.empty(L, k, dtype=F64, device=device), Y=torch.empty(L, H, k, dtype=F64, device=device))
            KN.tiled_paths_fwd([job], theta, method, H, K, m)
            out = dict(gx=gx if whole else torch.empty(d, k, dtype=F64, device=device), gs=gs[lo:lo + k], ut=ut[lo:lo + k])
            KN.tiled_paths_grad([dict(job, **out)], theta, method, H, K, m)
            u[lo:lo + k] = job['u'][L - 1]
            if not whole:
                gx[:, lo:lo + k] = out['gx']
        inv = inverse.to(device)
        grad = gx.t()[inv] + gs[inv].view(-1, 1) * hx.to(device)
        return dict(u=u[inv], grad=grad.contiguous(), ut=ut[inv])


# ---- parameter gradients: a weighted sum over the cloud of dU_p/dtheta -------------------------------------------------------------
def vjp_chunk_paths(chunk, L, H, P):
    """paths per launch of evaluate_points_vjp: a chunk's checkpoints Y [L, H, n] and its slabs [tiles, P] (P = theta's size) stay
    below EVAL_GRAD_CKPT_BYTES together, 8 (L H n + P tiles) with n = 16 tiles (whole 16-path tiles, at least one) -- a memory
    bound, not a tuned number.  At wide networks the slabs are the larger term: about 2 MB per tile at (256, 256)."""
    return min(chunk, 16 * max(1, EVAL_GRAD_CKPT_BYTES // (8 * (16 * L * H + P))))


def vjp_refuse_solver(solver):
    """XnwanError for the solvers evaluate_points_vjp does not serve (XNODE.evaluate_fn asks before its forward runs)"""
    if solver in REFUSED_SOLVERS:
        raise XnwanError("evaluate_vjp(): solver %r is not served -- parameter gradients at scattered points run the fixed-grid "
                         "schemes %s only (the reverse of the steps taken, with slabs; no per-path record sweep with slabs or "
                         "multistep history is built)" % (solver, sorted(KN.METHODS)))


def evaluate_points_vjp(points, w, n_sub, setup, domain, solver, h, theta, method, H, K, m, device, chunk=EVAL_CHUNK_PATHS):
    """u_theta at points [M, 1 + d] (time first; host or device, float32 or float64) and the weighted sum of its PARAMETER gradients,
    with weights w [M] -> dict(u [M], gflat [P_u], start [M]), float64 on `device`.  Entry rule, step counts, packing, sort and
    refusals are evaluate_points_grad's; per chunk (vjp_chunk_paths) kernels.tiled_paths_fwd keeps the checkpoints,
    kernels.tiled_paths_vjp walks them back and kernels.slab_sum adds the chunk's slabs to gflat:
      u      the forward's last row: the bits of evaluate_points
      gflat  sum_p w_p dU_p/dtheta in theta's layout (P_u = theta's size), U_p the DISCRETE solution at point p: the exact reverse
             of the steps taken, every point's grid and step sizes held fixed, the start value h([T0, x]) a constant of theta, ReLU
             kinks as autograd takes them.  The chunks go in sorted order, so its bits are a function of the inputs and `chunk`.
             Exact zeros for an empty cloud.
      start  w_p dU_p/dstart_p, the cotangent that reaches every point's start value (h itself is not differentiated)
    Refused: the solvers 'dopri5' and 'explicit_adams', a domain class without `entry`, t < t_in, every point that is not entered
    at T0 -- its start value g does not depend on theta either, but one rule holds for all gradients at scattered points --, and a
    w of another shape than [M].  No collective calls, no random numbers."""
    who = 'evaluate_vjp()'
    vjp_refuse_solver(solver)
    entry = getattr(domain, 'entry', None)
    if entry is None:
        name = getattr(domain, '__name__', type(domain).__name__)
        raise XnwanError('%s: the domain class %s has no entry(points, shape_param, T0, T) rule: where a point\'s path '
                         'starts, and with which start value, is the domain\'s to say' % (who, name))
    d, T0, T = setup['dim'], setup['T0'], setup['T']
    n_sub = setup['N_t'] if n_sub is None else n_sub
    if n_sub < 1:
        raise XnwanError('%s: n_sub = %r, at least one step over [T0, T]' % (who, n_sub))
    if chunk < 1:
        raise XnwanError('eval_chunk_paths = %d: at least one path per launch' % chunk)
    if not (torch.is_tensor(points) and points.dim() == 2 and points.shape[1] == 1 + d):
        raise XnwanError('%s: points must be a tensor [M, 1 + d] = [M, %d], time first' % (who, 1 + d))
    M = points.shape[0]
    if not (torch.is_tensor(w) and tuple(w.shape) == (M,)):
        raise XnwanError('%s: w must be a tensor [M] = [%d], a weight per point (got %s)'
                         % (who, M, tuple(w.shape) if torch.is_tensor(w) else type(w).__name__))
    P = KN.theta_size(d, H, K)
    with torch.no_grad():
        pts = points.detach().to(F64)
        gflat = torch.zeros(P, dtype=F64, device=device)
        if M == 0:
            return dict(u=torch.empty(0, dtype=F64, device=device), gflat=gflat, start=torch.empty(0, dtype=F64, device=device))
        t = pts[:, 0].contiguous()
        t_in, at_T0 = entry(pts, setup['shape_param'], T0, T)
        early = t < t_in
        if bool(early.any()):
            i = int(early.nonzero()[0])
            raise XnwanError('%s: %d points lie before their entry time (t >= t_in is the limit; first: point %d, '
                             't = %r, t_in = %r)' % (who, int(early.sum()), i, float(t[i]), float(t_in[i])))
        late = ~at_T0
        if bool(late.any()):
            i = int(late.nonzero()[0])
            raise XnwanError('%s: %d points are not entered at T0 (entry at T0 is the limit; first: point %d, t = %r, '
                             't_in = %r): their path starts on the moving boundary; the start value there does not depend on theta, '
                             'but gradients at scattered points keep one rule, evaluate_grad()\'s'
                             % (who, int(late.sum()), i, float(t[i]), float(t_in[i])))
        first = torch.cat((t_in.view(-1, 1), pts[:, 1:]), 1)
        s = h(first).reshape(-1).double()
        n = step_counts(t, t_in, T0, T, n_sub)
        order, inverse = sort_by_steps(n)
        tT = pack_grids(t[order], t_in[order], n[order]).to(device)
        xT = pts[order, 1:].t().contiguous().to(device)
        start, nstep = s[order].contiguous().to(device), n[order].to(torch.int32).to(device)
        ws = w.detach().to(F64).to(order.device)[order].contiguous().to(device)
        L = tT.shape[0]
        per = vjp_chunk_paths(chunk, L, H, P)
        u = torch.empty(M, dtype=F64, device=device)
        gs = torch.empty(M, dtype=F64, device=device)
        for lo in range(0, M, per):
            k = min(lo + per, M) - lo
            whole = k == M
            job = dict(xT=xT if whole else xT[:, lo:lo + k].contiguous(), start=start[lo:lo + k],
                       tT=tT if whole else tT[:, lo:lo + k].contiguous(), nstep=nstep[lo:lo + k],
                       u=torch.empty(L, k, dtype=F64, device=device), Y=torch.empty(L, H, k, dtype=F64, device=device))
            KN.tiled_paths_fwd([job], theta, method, H, K, m)
            gslab = torch.empty((k + 15) // 16, P, dtype=F64, device=device)
            KN.tiled_paths_vjp([dict(job, w=ws[lo:lo + k], gslab=gslab, gs=gs[lo:lo + k])], theta, method, H, K, m)
            KN.slab_sum(gslab, out=gflat, accumulate=True)
            u[lo:lo + k] = job['u'][L - 1]
        inv = inverse.to(device)
        return dict(u=u[inv], gflat=gflat, start=gs[inv])


def start_hvp(h, first, v):
    """(d^2h/dx^2 . v) [M, d] at first = [t_in, x] ([M, 1 + d]) for directions v [M, d]: double backward on a leaf copy of `first`
    -- the gradient of h(first).sum() with its graph kept, then the gradient of (that gradient . v).sum() -- the time column
    dropped.  It rests on start_gradient's assumption: h acts POINT BY POINT, so the sums decouple row by row.  Exact zeros where h
    or its gradient does not depend on its input (a constant h, an h that ignores x, an h that is linear in x)."""
    zero = torch.zeros_like(first[:, 1:])
    with torch.enable_grad():
        leaf = first.detach().clone().requires_grad_(True)
        out = h(leaf)
        if not (torch.is_tensor(out) and out.requires_grad):
            return zero
        grad, = torch.autograd.grad(out.sum(), leaf, create_graph=True, allow_unused=True)
        if grad is None or not grad.requires_grad:
            return zero
        hv, = torch.autograd.grad((grad[:, 1:] * v.detach().to(grad.dtype).to(grad.device)).sum(), leaf, allow_unused=True)
    if hv is None:
        return zero
    return hv[:, 1:].detach().to(first.dtype)


def hvp_chunk_paths(chunk, L, H):
    """paths per launch of evaluate_points_hvp / evaluate_points_hess: the checkpoints Y and the tangent checkpoints Yd, [L, H, n]
    each, stay below EVAL_GRAD_CKPT_BYTES together (whole 16-path tiles, at least one) -- a memory bound, not a tuned number"""
    return min(chunk, max(16, 16 * (EVAL_GRAD_CKPT_BYTES // (2 * 8 * L * H * 16))))


def second_order_entry(who, points, n_sub, setup, domain, solver, h, device, chunk):
    """the host side evaluate_points_hvp and evaluate_points_hess share, evaluate_points_grad's for the fixed-grid schemes: the
    refusals (under the name `who`), the entry rule, the start values and their gradient, step counts, packing and sort.
    -> None for an empty cloud, else a namespace of the sorted group on `device` and what puts results back"""
    if solver in REFUSED_SOLVERS:
        raise XnwanError("%s: solver %r is not served -- second derivatives at scattered points run the fixed-grid schemes %s only "
                         "(the tangent of the reverse sweep over the steps taken; no per-path step controller or multistep history "
                         "is differentiated twice)" % (who, solver, sorted(KN.METHODS)))
    entry = getattr(domain, 'entry', None)
    if entry is None:
        name = getattr(domain, '__name__', type(domain).__name__)
        raise XnwanError('%s: the domain class %s has no entry(points, shape_param, T0, T) rule: where a point\'s path '
                         'starts, and with which start value, is the domain\'s to say' % (who, name))
    d, T0, T = setup['dim'], setup['T0'], setup['T']
    n_sub = setup['N_t'] if n_sub is None else n_sub
    if n_sub < 1:
        raise XnwanError('%s: n_sub = %r, at least one step over [T0, T]' % (who, n_sub))
    if chunk < 1:
        raise XnwanError('eval_chunk_paths = %d: at least one path per launch' % chunk)
    if not (torch.is_tensor(points) and points.dim() == 2 and points.shape[1] == 1 + d):
        raise XnwanError('%s: points must be a tensor [M, 1 + d] = [M, %d], time first' % (who, 1 + d))
    pts = points.detach().to(F64)
    if pts.shape[0] == 0:
        return None
    t = pts[:, 0].contiguous()
    t_in, at_T0 = entry(pts, setup['shape_param'], T0, T)
    early = t < t_in
    if bool(early.any()):
        i = int(early.nonzero()[0])
        raise XnwanError('%s: %d points lie before their entry time (t >= t_in is the limit; first: point %d, '
                         't = %r, t_in = %r)' % (who, int(early.sum()), i, float(t[i]), float(t_in[i])))
    late = ~at_T0
    if bool(late.any()):
        i = int(late.nonzero()[0])
        raise XnwanError('%s: %d points are not entered at T0 (entry at T0 is the limit; first: point %d, t = %r, '
                         't_in = %r): their path starts on the moving boundary at a time that depends on x, and derivatives '
                         'with that time held fixed are not those of u in x' % (who, int(late.sum()), i, float(t[i]), float(t_in[i])))
    first = torch.cat((t_in.view(-1, 1), pts[:, 1:]), 1)
    s = h(first).reshape(-1).double()
    n = step_counts(t, t_in, T0, T, n_sub)
    order, inverse = sort_by_steps(n)
    return types.SimpleNamespace(
        M=pts.shape[0], d=d, first=first, dh=start_gradient(h, first).to(F64), order=order, inv=inverse.to(device),
        tT=pack_grids(t[order], t_in[order], n[order]).to(device), xT=pts[order, 1:].t().contiguous().to(device),
        start=s[order].contiguous().to(device), nstep=n[order].to(torch.int32).to(device))


def second_order_pass(e, ndir, direction, theta, method, H, K, m, device, chunk, want_ju=False):
    """per chunk of the sorted group e (second_order_entry): kernels.tiled_paths_fwd with its checkpoints kept,
    kernels.tiled_paths_grad for gx and gs, then one kernels.tiled_paths_hvp launch per direction i < ndir over the same
    checkpoints, the tangent checkpoints and the workspace shared by the directions.  direction(i, lo, k) -> (vxT [d, k], vs [k]),
    contiguous on the device, for the chunk's paths lo .. lo + k of the sorted group: a direction exists for one chunk at a time.
    -> (u [M], gx [d, M], gs [M], ju [ndir, M] or None, hx [ndir, d, M], hs [ndir, M]), sorted as e"""
    M, d, L = e.M, e.d, e.tT.shape[0]
    per = hvp_chunk_paths(chunk, L, H)
    new = lambda *shape: torch.empty(*shape, dtype=F64, device=device)   # noqa: E731
    u, gx, gs = new(M), new(d, M), new(M)
    ju, hx, hs = new(ndir, M) if want_ju else None, new(ndir, d, M), new(ndir, M)
    for lo in range(0, M, per):
        k = min(lo + per, M) - lo
        whole = k == M
        cut = (lambda a: a) if whole else (lambda a: a[:, lo:lo + k].contiguous())
        job = dict(xT=cut(e.xT), start=e.start[lo:lo + k], tT=cut(e.tT), nstep=e.nstep[lo:lo + k], u=new(L, k), Y=new(L, H, k))
        KN.tiled_paths_fwd([job], theta, method, H, K, m)
        g = dict(gx=gx if whole else new(d, k), gs=gs[lo:lo + k])
        KN.tiled_paths_grad([dict(job, **g)], theta, method, H, K, m)
        u[lo:lo + k] = job['u'][L - 1]
        if not whole:
            gx[:, lo:lo + k] = g['gx']
        Yd, work = new(L, H, k), KN.paths_hvp_work(d, H, K, m, (k + 15) // 16, device)
        part = None if whole else new(d, k)
        for i in range(ndir):
            vxT, vs = direction(i, lo, k)
            o = dict(vx=vxT, vs=vs, Yd=Yd, hx=hx[i] if whole else part, hs=hs[i, lo:lo + k])
            if want_ju:
                o['ju'] = ju[i, lo:lo + k]
            KN.tiled_paths_hvp([dict(job, **o)], theta, method, H, K, m, work=work)
            if not whole:
                hx[i, :, lo:lo + k] = part
    return u, gx, gs, ju, hx, hs


def evaluate_points_hvp(points, v, n_sub, setup, domain, solver, h, theta, method, H, K, m, device, chunk=EVAL_CHUNK_PATHS):
    """u_theta, its gradient in x and its Hessian in x applied to a direction per point, at points [M, 1 + d] (time first; host or
    device, float32 or float64) with v [M, d] -> dict(u [M], grad [M, d], dv [M], hvp [M, d]), float64 on `device`.  Entry rule,
    step counts, packing, sort and refusals are evaluate_points_grad's; per chunk (hvp_chunk_paths) three launches: the forward
    with its checkpoints kept, kernels.tiled_paths_grad, and kernels.tiled_paths_hvp with the direction (v, dh/dx . v):
      u, grad  the bits of evaluate_points_grad
      dv       grad . v, the directional derivative, from the tangent forward (ju)
      hvp      d/dx (du/dx) . v of the DISCRETE solution x -> U(x, h([T0, x])) with every point's grid held fixed:
               hx + hs dh/dx + gs (d^2h/dx^2 . v) (start_gradient, start_hvp: the chain rule through the start value); ReLU kinks
               as autograd takes them.
    Time is not perturbed.  Refused: the solvers 'dopri5' and 'explicit_adams', a domain class without `entry`, t < t_in, every
    point that is not entered at T0, and a v of another shape than [M, d].  No collective calls, no random numbers."""
    who = 'evaluate_hvp()'
    with torch.no_grad():
        e = second_order_entry(who, points, n_sub, setup, domain, solver, h, device, chunk)
        M, d = points.shape[0], setup['dim']
        if not (torch.is_tensor(v) and tuple(v.shape) == (M, d)):
            raise XnwanError('%s: v must be a tensor [M, d] = [%d, %d], a direction per point (got %s)'
                             % (who, M, d, tuple(v.shape) if torch.is_tensor(v) else type(v).__name__))
        if e is None:
            new = lambda *shape: torch.empty(*shape, dtype=F64, device=device)   # noqa: E731
            return dict(u=new(0), grad=new(0, d), dv=new(0), hvp=new(0, d))
        vv = v.detach().to(F64).to(e.first.device)
        d2 = start_hvp(h, e.first, vv).to(F64).to(device)
        dh = e.dh.to(device)
        vd = vv.to(device)
        od = e.order.to(device)
        vxT, vs = vd[od].t().contiguous(), (dh * vd).sum(1)[od].contiguous()
        direction = lambda i, lo, k: (vxT if k == M else vxT[:, lo:lo + k].contiguous(), vs[lo:lo + k])   # noqa: E731
        u, gx, gs, ju, hx, hs = second_order_pass(e, 1, direction, theta, method, H, K, m, device, chunk, want_ju=True)
        inv = e.inv
        grad = gx.t()[inv] + gs[inv].view(-1, 1) * dh
        hvp = hx[0].t()[inv] + hs[0][inv].view(-1, 1) * dh + gs[inv].view(-1, 1) * d2
        return dict(u=u[inv], grad=grad.contiguous(), dv=ju[0][inv], hvp=hvp.contiguous())


# ---- parameter gradients of u, du/dx and ut: a weighted sum over the cloud ----------------------------------------------------------
def gvjp_chunk_paths(chunk, L, H, P):
    """paths per launch of evaluate_points_grad_vjp: a chunk's checkpoints Y and tangent checkpoints Yd, [L, H, n] each, and its
    slabs [tiles, P] (P = theta's size) stay below EVAL_GRAD_CKPT_BYTES together, 8 (2 L H n + P tiles) with n = 16 tiles (whole
    16-path tiles, at least one) -- a memory bound, not a tuned number"""
    return min(chunk, 16 * max(1, EVAL_GRAD_CKPT_BYTES // (8 * (2 * 16 * L * H + P))))


def grad_vjp_refuse_solver(solver):
    """XnwanError for the solvers evaluate_points_grad_vjp does not serve (XNODE.evaluate_grad_fn asks before its forward runs)"""
    if solver in REFUSED_SOLVERS:
        raise XnwanError("evaluate_grad_vjp(): solver %r is not served -- parameter gradients of du/dx and ut at scattered points run "
                         "the fixed-grid schemes %s only (the tangent of the reverse of the steps taken, with slabs; no per-path "
                         "record sweep or multistep history is differentiated twice)" % (solver, sorted(KN.METHODS)))


def evaluate_points_grad_vjp(points, wu, wg, wt, n_sub, setup, domain, solver, h, theta, method, H, K, m, device,
                             chunk=EVAL_CHUNK_PATHS):
    """u_theta, its gradient in x and its time derivative at points [M, 1 + d] (time first; host or device, float32 or float64) and
    the PARAMETER gradient of their weighted sum, with weights wu [M], wg [M, d], wt [M] (each may be None: zeros; not all three)
    -> dict(u [M], grad [M, d], ut [M], gflat [P_u]), float64 on `device`.  Entry rule, refusals, step counts, packing and sort are
    second_order_entry's; per chunk (gvjp_chunk_paths) kernels.tiled_paths_fwd keeps the checkpoints, kernels.tiled_paths_grad gives
    grad and ut, kernels.tiled_paths_hvp with ju alone runs the tangent forward along (wg, dh/dx . wg), kernels.tiled_paths_gvjp
    walks both sets of checkpoints back and kernels.slab_sum adds the chunk's slabs to gflat:
      u, grad, ut  the bits of evaluate_points_grad
      gflat        d/dtheta sum_p [wu_p U_p + wg_p . dU_p/dx + wt_p ut_p] in theta's layout (P_u = theta's size).  U_p is the DISCRETE
                   solution at point p as evaluate_points_vjp differentiates it: every point's grid and step sizes held fixed, the
                   start value h([T0, x]) AND its gradient dh/dx constants of theta, ReLU kinks as autograd takes them; dU_p/dx is
                   evaluate_points_grad's grad, gx + gs dh/dx, so wg_p . dU_p/dx is the derivative of (x, s) -> U_p along
                   (wg_p, dh/dx . wg_p).  ut_p = FL_w . F(t_p, x_p, y(t_p)) belongs to the CONTINUOUS model; theta enters it through
                   the read-out, the field and y(t_p), the last by the same discrete reverse.  The chunks go in sorted order, so the
                   bits are a function of the inputs and `chunk`.  Exact zeros for an empty cloud.
    Refused: the solvers 'dopri5' and 'explicit_adams', a domain class without `entry`, t < t_in, every point that is not entered
    at T0, wu, wg and wt all None, and a weight of another shape.  No collective calls, no random numbers."""
    who = 'evaluate_grad_vjp()'
    grad_vjp_refuse_solver(solver)
    with torch.no_grad():
        e = second_order_entry(who, points, n_sub, setup, domain, solver, h, device, chunk)
        M, d = points.shape[0], setup['dim']
        if wu is None and wg is None and wt is None:
            raise XnwanError('%s: nothing to differentiate: at least one of wu [M], wg [M, d], wt [M] must be given' % who)
        for name, a, shape in (('wu', wu, (M,)), ('wg', wg, (M, d)), ('wt', wt, (M,))):
            if a is not None and not (torch.is_tensor(a) and tuple(a.shape) == shape):
                raise XnwanError('%s: %s must be None or a tensor %s, a weight per point (got %s)'
                                 % (who, name, list(shape), tuple(a.shape) if torch.is_tensor(a) else type(a).__name__))
        P = KN.theta_size(d, H, K)
        new = lambda *shape: torch.empty(*shape, dtype=F64, device=device)   # noqa: E731
        gflat = torch.zeros(P, dtype=F64, device=device)
        if e is None:
            return dict(u=new(0), grad=new(0, d), ut=new(0), gflat=gflat)
        od, dh = e.order.to(device), e.dh.to(device)
        sort = lambda a: None if a is None else a.detach().to(F64).to(device)[od].contiguous()   # noqa: E731
        wus, wts = sort(wu), sort(wt)
        vxT = vs = None
        if wg is not None:
            vd = wg.detach().to(F64).to(device)
            vxT, vs = vd[od].t().contiguous(), (dh * vd).sum(1)[od].contiguous()
        L = e.tT.shape[0]
        per = gvjp_chunk_paths(chunk, L, H, P)
        u, gx, gs, ut = new(M), new(d, M), new(M), new(M)
        for lo in range(0, M, per):
            k = min(lo + per, M) - lo
            whole = k == M
            cut = (lambda a: a) if whole else (lambda a: a[:, lo:lo + k].contiguous())
            job = dict(xT=cut(e.xT), start=e.start[lo:lo + k], tT=cut(e.tT), nstep=e.nstep[lo:lo + k], u=new(L, k), Y=new(L, H, k))
            KN.tiled_paths_fwd([job], theta, method, H, K, m)
            g = dict(gx=gx if whole else new(d, k), gs=gs[lo:lo + k], ut=ut[lo:lo + k])
            KN.tiled_paths_grad([dict(job, **g)], theta, method, H, K, m)
            u[lo:lo + k] = job['u'][L - 1]
            if not whole:
                gx[:, lo:lo + k] = g['gx']
            tiles = (k + 15) // 16
            o = dict(gslab=new(tiles, P))
            if wus is not None:
                o['wu'] = wus[lo:lo + k]
            if wts is not None:
                o['wt'] = wts[lo:lo + k]
            if vxT is not None:
                o.update(vx=cut(vxT), vs=vs[lo:lo + k], Yd=new(L, H, k))
                KN.tiled_paths_hvp([dict(job, ju=new(k), **{n: o[n] for n in ('vx', 'vs', 'Yd')})], theta, method, H, K, m)
            KN.tiled_paths_gvjp([dict(job, **o)], theta, method, H, K, m)
            KN.slab_sum(o['gslab'], out=gflat, accumulate=True)
        inv = e.inv
        grad = gx.t()[inv] + gs[inv].view(-1, 1) * dh
        return dict(u=u[inv], grad=grad.contiguous(), ut=ut[inv], gflat=gflat)


def evaluate_points_hess(points, n_sub, setup, domain, solver, h, theta, method, H, K, m, device, chunk=EVAL_CHUNK_PATHS):
    """u_theta, its gradient, its Hessian in x and its Laplacian at points [M, 1 + d] -> dict(u [M], grad [M, d], hess [M, d, d],
    lap [M]), float64 on `device`.  evaluate_points_hvp's chain with d directions: per chunk the forward and the gradient run once,
    then d launches of kernels.tiled_paths_hvp, v = e_k, over the same checkpoints; row k of hess is the k-th product,
    hx_k + hs_k dh/dx + gs (d^2h/dx^2 . e_k).  hess is NOT symmetrised: its asymmetry is rounding, and a check.  lap is its trace.
    Memory besides the chunk's checkpoints: the products as the launches write them ([d, d, M], the size of hess) and one unit
    direction [d, chunk] that is refilled; d^2h/dx^2 . e_k is taken one k at a time.  Refusals: evaluate_points_hvp's."""
    who = 'evaluate_hess()'
    with torch.no_grad():
        e = second_order_entry(who, points, n_sub, setup, domain, solver, h, device, chunk)
        d = setup['dim']
        if e is None:
            new = lambda *shape: torch.empty(*shape, dtype=F64, device=device)   # noqa: E731
            return dict(u=new(0), grad=new(0, d), hess=new(0, d, d), lap=new(0))
        dh = e.dh.to(device)
        dhs = dh[e.order.to(device)].t().contiguous()                # [d, M], sorted: row k is vs of direction e_k
        unit = {}

        def direction(i, lo, k):                                     # (refilled on the launches' stream, so in their order)
            if unit.get('k') != k:
                unit['k'], unit['e'] = k, torch.empty(d, k, dtype=F64, device=device)
            unit['e'].zero_()
            unit['e'][i].fill_(1.0)
            return unit['e'], dhs[i, lo:lo + k]
        u, gx, gs, _, hx, hs = second_order_pass(e, d, direction, theta, method, H, K, m, device, chunk)
        inv = e.inv
        gsi = gs[inv].view(-1, 1)
        grad = gx.t()[inv] + gsi * dh
        hess = hx.permute(2, 0, 1)[inv]                              # [M, d, d]: row k = hx of direction e_k
        del hx
        hess += hs.t()[inv].unsqueeze(2) * dh.unsqueeze(1)
        eye = torch.eye(d, dtype=F64, device=e.first.device)
        for k in range(d):
            hess[:, k, :] += gsi * start_hvp(h, e.first, eye[k].expand(e.M, d)).to(F64).to(device)
        return dict(u=u[inv], grad=grad.contiguous(), hess=hess.contiguous(), lap=torch.diagonal(hess, dim1=1, dim2=2).sum(1))


def evaluate_points(points, n_sub, setup, domain, solver, h, g, theta, method, H, K, m, device, chunk=EVAL_CHUNK_PATHS, tol=None,
                    Hn=None, max_steps=KN.DOPRI5_MAX_STEPS):
    """u_theta at points [M, 1 + d] (time first; host or device, float32 or float64) -> u [M] float64 on `device`.
    domain: the domain class or an instance (only its classmethod `entry` is used: nothing is constructed, nothing is drawn).
    tol = (rtol, atol) with solver 'dopri5': every point is one adaptive solve of its own from its entry to t, a step controller
    per path (paths_dopri5; Hn: the network's u_hidden_dim, H unless given; max_steps: accepted steps per path); n_sub has no
    meaning there and must be None.  A path whose controller ends with a status raises XnwanError."""
    adaptive = solver == 'dopri5' and tol is not None
    if solver in REFUSED_SOLVERS and not adaptive:
        raise XnwanError("evaluate(): solver %r is not served -- per-path time grids run the fixed-grid schemes %s only (no "
                         "per-path step controller or multistep history is built)" % (solver, sorted(KN.METHODS)))
    if adaptive and n_sub is not None:
        raise XnwanError("evaluate(): n_sub = %r with solver 'dopri5' -- every point's step sizes are its controller's (rtol, atol); "
                         "a number of steps over [T0, T] has no meaning there" % (n_sub,))
    entry = getattr(domain, 'entry', None)
    if entry is None:
        name = getattr(domain, '__name__', type(domain).__name__)
        raise XnwanError('evaluate(): the domain class %s has no entry(points, shape_param, T0, T) rule: where a point\'s path '
                         'starts, and with which start value, is the domain\'s to say' % name)
    d, T0, T = setup['dim'], setup['T0'], setup['T']
    n_sub = setup['N_t'] if n_sub is None else n_sub
    if not adaptive and n_sub < 1:
        raise XnwanError('evaluate(): n_sub = %r, at least one step over [T0, T]' % (n_sub,))
    if not (torch.is_tensor(points) and points.dim() == 2 and points.shape[1] == 1 + d):
        raise XnwanError('evaluate(): points must be a tensor [M, 1 + d] = [M, %d], time first' % (1 + d))
    with torch.no_grad():
        pts = points.detach().to(F64)
        if pts.shape[0] == 0:
            return torch.empty(0, dtype=F64, device=device)
        t = pts[:, 0].contiguous()
        t_in, at_T0 = entry(pts, setup['shape_param'], T0, T)
        early = t < t_in
        if bool(early.any()):
            i = int(early.nonzero()[0])
            raise XnwanError('evaluate(): %d points lie before their entry time (t >= t_in is the limit; first: point %d, t = %r, '
                             't_in = %r)' % (int(early.sum()), i, float(t[i]), float(t_in[i])))
        first = torch.cat((t_in.view(-1, 1), pts[:, 1:]), 1)
        if bool(at_T0.all()):
            s = h(first).reshape(-1).double()
        else:                               # (both callables on every point, then a select: the batched form of h(x0) / g(x0))
            s = torch.where(at_T0, h(first).reshape(-1).double(), g(first.unsqueeze(1)).reshape(-1).double())
        if adaptive:
            # sorted by the length of the interval -- what a path's step count grows with; the count itself is the controller's --
            # so that the 16 paths of a tile, which walk together until the last of them is done, need about the same rounds
            order, inverse = sort_by_steps(t - t_in)
            r = paths_dopri5(pts[order, 1:].t().contiguous().to(device), t_in[order].contiguous().to(device),
                             t[order].contiguous().to(device), s[order].contiguous().to(device), theta, H, K, m,
                             H if Hn is None else Hn, float(tol[0]), float(tol[1]), max_steps=max_steps, chunk=chunk)
            raise_unreached('evaluate()', r, order, inverse, t, t_in, max_steps)
            return r['u'][inverse.to(device)]
        n = step_counts(t, t_in, T0, T, n_sub)
        order, inverse = sort_by_steps(n)
        tT = pack_grids(t[order], t_in[order], n[order]).to(device)
        u = paths_forward(pts[order, 1:].t().contiguous().to(device), tT, s[order].contiguous().to(device),
                          n[order].to(torch.int32).to(device), theta, method, H, K, m, last_only=True, chunk=chunk)
        return u[inverse.to(device)]


# ---- second-order forward jets: quadratic forms of the Hessian, the diffusion term and the strong-form residual ------------------------
def jet_chunk_paths(chunk, R, work):
    """paths per launch of evaluate_points_quad / evaluate_points_lap with R directions per path and `work` doubles of workspace per
    block (kernels.paths_jet_work: a block per tile and direction): tiles * R * work * 8 <= EVAL_GRAD_CKPT_BYTES, whole 16-path
    tiles, at least one -- a memory bound, not a tuned number.  There are no checkpoints: the workspace is what grows."""
    return min(chunk, 16 * max(1, EVAL_GRAD_CKPT_BYTES // (8 * R * work)))


def lap_directions(a, M, d, who='evaluate_lap()'):
    """directions and weights (Q, lam) with sum_ij a_ij H_ij = sum_k lam_k q_k^T H q_k for every symmetric H: Q [R, d] and lam [R]
    where one set serves all points, Q [M, R, d] and lam [M, R] where a point has its own; R = d, float64 on a's device (None: the
    host).  a None: the unit directions with weights 1.  a [d, d] or [M, d, d] with every off-diagonal entry exactly zero: the unit
    directions with weights a_kk.  Otherwise torch.linalg.eigh of the symmetric part (a_ij + a_ji) / 2 -- the antisymmetric part
    contracts to zero with a Hessian --, on the host: rows q_k the eigenvectors, lam_k the eigenvalues; one decomposition for a
    [d, d] matrix.  Another shape is refused."""
    if a is None:
        return torch.eye(d, dtype=F64), torch.ones(d, dtype=F64)
    if not (torch.is_tensor(a) and tuple(a.shape) in ((d, d), (M, d, d))):
        raise XnwanError('%s: a must be None (the Laplacian) or a tensor [d, d] = [%d, %d] or [M, d, d] = [%d, %d, %d] (got %s)'
                         % (who, d, d, M, d, d, tuple(a.shape) if torch.is_tensor(a) else type(a).__name__))
    A = a.detach().to(F64)
    diag = torch.diagonal(A, dim1=-2, dim2=-1)
    if bool(torch.all(A - torch.diag_embed(diag) == 0)):
        return torch.eye(d, dtype=F64, device=A.device), diag.contiguous()
    lam, Qm = torch.linalg.eigh((0.5 * (A + A.transpose(-1, -2))).cpu())
    return Qm.transpose(-1, -2).contiguous().to(A.device), lam.to(A.device)


def quad_pass(e, V, h, theta, method, H, K, m, device, chunk):
    """kernels.tiled_paths_jet over the sorted group e (second_order_entry) with the directions V -- [R, d], one set for all points,
    or [M, R, d], in the caller's order -- and the chain rule through the start value: per direction vs = dh/dx . v and
    qs = v . (d^2h/dx^2 . v) (start_gradient, start_hvp).  Per chunk (jet_chunk_paths) ONE launch, a block per tile and direction.
    -> (u [M], ju [R, M], quu [R, M]), in the caller's order"""
    M, d, R = e.M, e.d, V.shape[-2]
    shared = V.dim() == 2
    Vh = V.detach().to(F64).to(e.first.device)
    vs, qs = [], []
    for r in range(R):
        v = Vh[r].expand(M, d) if shared else Vh[:, r]
        vs.append((e.dh * v).sum(1))
        qs.append((v * start_hvp(h, e.first, v).to(F64)).sum(1))
    od = e.order.to(device)
    vs, qs = torch.stack(vs)[:, e.order].contiguous().to(device), torch.stack(qs)[:, e.order].contiguous().to(device)
    Vd = Vh.to(device)
    doubles = KN.lib.xw_paths_tiled_jet_work(d, H, K, m)
    KN.check(min(doubles, 0), 'xw_paths_tiled_jet_work')
    per = jet_chunk_paths(chunk, R, doubles)
    new = lambda *shape: torch.empty(*shape, dtype=F64, device=device)   # noqa: E731
    u, ju, quu = new(M), new(R, M), new(R, M)
    work, vx = None, None
    for lo in range(0, M, per):
        k = min(lo + per, M) - lo
        whole = k == M
        cut = (lambda a: a) if whole else (lambda a: a[:, lo:lo + k].contiguous())
        if not shared:
            vx = Vd[od[lo:lo + k]].permute(1, 2, 0).contiguous()
        elif vx is None or vx.shape[2] != k:
            vx = Vd.unsqueeze(2).expand(R, d, k).contiguous()
        if work is None or work.numel() != doubles * R * ((k + 15) // 16):   # (the chunks share it: they share the stream)
            work = KN.paths_jet_work(d, H, K, m, R * ((k + 15) // 16), device)
        out = dict(u=u[lo:lo + k], ju=ju if whole else new(R, k), quu=quu if whole else new(R, k))
        KN.tiled_paths_jet([dict(xT=cut(e.xT), start=e.start[lo:lo + k], tT=cut(e.tT), nstep=e.nstep[lo:lo + k], vx=vx, vs=cut(vs),
                                 qs=cut(qs), **out)], theta, method, H, K, m, work=work)
        if not whole:
            ju[:, lo:lo + k], quu[:, lo:lo + k] = out['ju'], out['quu']
    return u[e.inv], ju[:, e.inv], quu[:, e.inv]


def evaluate_points_quad(points, V, n_sub, setup, domain, solver, h, theta, method, H, K, m, device, chunk=EVAL_CHUNK_PATHS):
    """u_theta and, along R directions per point, its first and second directional derivatives in x, at points [M, 1 + d] (time
    first; host or device, float32 or float64) with V [M, R, d] -> dict(u [M], dv [M, R], quad [M, R]), float64 on `device`.  Entry
    rule, step counts, packing, sort and refusals are evaluate_points_hvp's (second_order_entry); per chunk (jet_chunk_paths) ONE
    launch of kernels.tiled_paths_jet, a second-order forward jet: no reverse sweep, no checkpoints, nothing of size [M, d, d].
      u     the kernel's own, the bits of evaluate_points (the jet's primal runs the forward's step text on the forward's blocks)
      dv    grad . v_r, the directional derivative
      quad  v_r^T (d^2u/dx^2) v_r of the DISCRETE solution x -> U(x, h([T0, x])) with every point's grid held fixed: the second
            derivative of eps -> U(x + eps v, h(x + eps v)) at 0, the chain rule through the start value to second order
            (vs = dh/dx . v, qs = v . d^2h/dx^2 v); ReLU kinks as autograd takes them.
    Time is not perturbed.  Refused: the solvers 'dopri5' and 'explicit_adams', a domain class without `entry`, t < t_in, every
    point that is not entered at T0, and a V of another shape than [M, R, d] with R >= 1.  No collective calls, no random numbers."""
    who = 'evaluate_quad()'
    with torch.no_grad():
        e = second_order_entry(who, points, n_sub, setup, domain, solver, h, device, chunk)
        M, d = points.shape[0], setup['dim']
        if not (torch.is_tensor(V) and V.dim() == 3 and V.shape[0] == M and V.shape[1] >= 1 and V.shape[2] == d):
            raise XnwanError('%s: V must be a tensor [M, R, d] = [%d, R, %d], R >= 1 directions per point (got %s)'
                             % (who, M, d, tuple(V.shape) if torch.is_tensor(V) else type(V).__name__))
        R = V.shape[1]
        if e is None:
            new = lambda *shape: torch.empty(*shape, dtype=F64, device=device)   # noqa: E731
            return dict(u=new(0), dv=new(0, R), quad=new(0, R))
        u, ju, quu = quad_pass(e, V, h, theta, method, H, K, m, device, chunk)
        return dict(u=u, dv=ju.t().contiguous(), quad=quu.t().contiguous())


def evaluate_points_lap(points, a, n_sub, setup, domain, solver, h, theta, method, H, K, m, device, chunk=EVAL_CHUNK_PATHS,
                        who='evaluate_lap()'):
    """u_theta and the diffusion term lap = sum_ij a_ij d^2u/dx_i dx_j at points [M, 1 + d] -> dict(u [M], lap [M]), float64 on
    `device`: evaluate_points_quad's launch with the d directions and weights of lap_directions(a) -- a None: the Laplacian, the
    unit directions; a [d, d] or [M, d, d] (the coefficient tabulated per point) with exactly zero off-diagonal entries: the unit
    directions weighted by a_kk; otherwise the eigenvectors and eigenvalues of its symmetric part -- and lap = sum_k lam_k quad_k.
    Derivatives of the DISCRETE solution with every point's grid held fixed, as evaluate_points_quad states them; the route of
    evaluate_points_hess without the reverse sweeps, the checkpoints and the [M, d, d] output.  Refusals: evaluate_points_quad's,
    and an `a` of another shape."""
    with torch.no_grad():
        e = second_order_entry(who, points, n_sub, setup, domain, solver, h, device, chunk)
        M, d = points.shape[0], setup['dim']
        Q, lam = lap_directions(a, M, d, who)
        if e is None:
            return dict(u=torch.empty(0, dtype=F64, device=device), lap=torch.empty(0, dtype=F64, device=device))
        u, _, quu = quad_pass(e, Q, h, theta, method, H, K, m, device, chunk)
        lam = lam.to(device)
        lap = (quu * (lam.view(-1, 1) if lam.dim() == 1 else lam.t())).sum(0)
        return dict(u=u, lap=lap)


def divergence_a(func_a, X, d):
    """(div a)_j = sum_i d a_ij / d x_i on X [M, 1, 1 + d] -> [M, d], float64 on X's device: torch.autograd.grad of
    func_a(leaf, i, j).sum() with respect to a leaf copy of X, entry by entry (the callable is taken to act POINT BY POINT, as
    start_gradient takes h).  Exact zeros where an entry does not depend on X (no grad_fn, or an unused input)."""
    M = X.shape[0]
    div = torch.zeros(M, d, dtype=F64, device=X.device)
    with torch.enable_grad():
        leaf = X.detach().clone().requires_grad_(True)
        for i in range(d):
            for j in range(d):
                out = func_a(leaf, i, j)
                if not (torch.is_tensor(out) and out.requires_grad):
                    continue
                grad, = torch.autograd.grad(out.sum(), leaf, allow_unused=True)
                if grad is not None:
                    div[:, j] += grad.detach().reshape(M, -1)[:, 1 + i].to(F64)
    return div


def evaluate_points_residual(points, funcs, n_sub, setup, domain, solver, h, theta, method, H, K, m, device, chunk=EVAL_CHUNK_PATHS,
                             div_a='autograd'):
    """the strong-form residual of u_theta at points [M, 1 + d], for the PDE as the configs state it,
        du/dt - sum_i d_i (sum_j a_ij d_j u) + b . grad u + c u = f,   c = func_c(X, u):
    -> dict(u [M], ut [M], grad [M, d], diffusion [M], residual [M]), float64 on `device`, with
        residual = ut - diffusion - (div a) . grad + b . grad + c u - f,   diffusion = sum_ij a_ij d^2u/dx_i dx_j.
    funcs: dict(a, b, c, f) in the reference's callable protocol (func_a(X, i, j), func_b(X, i), func_f(X) -> [M, 1],
    func_c(X, u) -> [M, 1, 1]), tabulated in float64 on X = points.view(M, 1, 1 + d), where the points live.  u, ut and grad are
    evaluate_points_grad's, bit for bit; diffusion is evaluate_points_lap's with the tabulated a.  (div a)_j = sum_i d_i a_ij comes
    from autograd through func_a (divergence_a: exact zeros where an entry does not depend on X) unless div_a is a callable
    div_a(X, j) -> [M, 1].
    What the derivatives are: ut is the time derivative of the CONTINUOUS model, FL_w . F(t, x, y(t)); grad and diffusion are
    derivatives in x of the DISCRETE solution with every point's grid held fixed, as evaluate_points_grad documents -- the residual
    mixes the two and is a check of the trained u, not an identity of the scheme.  The reference's loss carries the source term as
    + f phi "as written"; the residual does not follow that sign: it is the PDE's, f on the right-hand side.
    Refusals: evaluate_points_quad's, under this function's name; a div_a that is neither 'autograd' nor callable."""
    who = 'evaluate_residual()'
    if not (div_a == 'autograd' or callable(div_a)):
        raise XnwanError("%s: div_a must be 'autograd' or a callable div_a(X, j) (got %r)" % (who, div_a))
    with torch.no_grad():
        d = setup['dim']
        if second_order_entry(who, points, n_sub, setup, domain, solver, h, device, chunk) is None:
            new = lambda *shape: torch.empty(*shape, dtype=F64, device=device)   # noqa: E731
            return dict(u=new(0), ut=new(0), grad=new(0, d), diffusion=new(0), residual=new(0))
        M = points.shape[0]
        X = points.detach().to(F64).view(M, 1, 1 + d)
        tab = lambda out: out.detach().to(F64).reshape(M).to(device)   # noqa: E731
        A = torch.stack([torch.stack([tab(funcs['a'](X, i, j)) for j in range(d)], 1) for i in range(d)], 1)     # [M, d, d]
        B = torch.stack([tab(funcs['b'](X, i)) for i in range(d)], 1)                                            # [M, d]
        if callable(div_a):
            D = torch.stack([tab(div_a(X, j)) for j in range(d)], 1)
        else:
            D = divergence_a(funcs['a'], X, d).to(device)
        g = evaluate_points_grad(points, n_sub, setup, domain, solver, h, theta, method, H, K, m, device, chunk=chunk)
        diffusion = evaluate_points_lap(points, A, n_sub, setup, domain, solver, h, theta, method, H, K, m, device, chunk=chunk,
                                        who=who)['lap']
        u, ut, grad = g['u'], g['ut'], g['grad']
        c = tab(funcs['c'](X, u.to(X.device).view(M, 1, 1)))
        f = tab(funcs['f'](X))
        residual = ut - diffusion - (D * grad).sum(1) + (B * grad).sum(1) + c * u - f
        return dict(u=u, ut=ut, grad=grad, diffusion=diffusion, residual=residual)
