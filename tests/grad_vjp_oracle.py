"""The reference of the parameter gradients of u, du/d(x, s) along a direction and ut (include/xnwan_grad_vjp.h), on the host:
oracle.refspec's arithmetic on ONE path under autograd.  For a path with the point x, the start value s, its own times, the
direction (vx, vs) and theta as a dict of the oracle's keys, three gradients in theta, each a dict key -> tensor (zeros where
autograd gives None):
  Gu  d/dtheta U,                          U = FL(y_n) the discrete final value
  Gd  d/dtheta (dU/dx . vx + dU/ds vs),    the direction a constant of theta
  Gt  d/dtheta ut,                         ut = FL_w . F(t_n, x, y_n), theta entering through FL_w, the field and y_n
reverse_over_reverse is the definition the device is held to: autograd in theta of the scalar, with create_graph on the gradient in
(x, s).  forward_over_reverse takes Gd another way -- torch.autograd.functional.jvp of (x, s) -> dU/dtheta along the direction --
and is the reference's own floor (tests/test_eval_grad_vjp_host.py).  Shared by the host and the device tests; not a test."""
import torch

F64 = torch.float64
U_ORDER = ['IL0_w', 'IL0_b', 'IL2_w', 'IL2_b', 'IL4_w', 'IL4_b', 'Win', 'Win_b', 'Wh', 'Wh_b', 'Wo', 'Wo_b', 'FL_w', 'FL_b']


def _final_state(R, th, m, method, xi, si, times):
    s = si.view(-1, 1)
    y0 = torch.relu(torch.relu(s @ th['IL0_w'].T + th['IL0_b']) @ th['IL2_w'].T + th['IL2_b']) @ th['IL4_w'].T + th['IL4_b']
    return R.odeint_fixed(lambda tt, y: R.field(th, m, xi, tt, y), y0, times, method)[0][-1:]


def _grads(scalar, th, **kw):
    if not scalar.requires_grad:
        return {k: torch.zeros_like(th[k]) for k in U_ORDER}
    g = torch.autograd.grad(scalar, [th[k] for k in U_ORDER], allow_unused=True, **kw)
    return {k: torch.zeros_like(th[k]) if a is None else a.detach() for k, a in zip(U_ORDER, g)}


def reverse_over_reverse(theta, m, method, x, s, times, vx, vs):
    """(Gu, Gd, Gt) of one path: x [d], s a scalar tensor, times [n + 1], vx [d], vs a scalar tensor"""
    from oracle import refspec as R
    th = {k: theta[k].detach().clone().requires_grad_(True) for k in U_ORDER}
    xi = x.detach().view(1, -1).clone().requires_grad_(True)
    si = s.detach().view(1).clone().requires_grad_(True)
    yT = _final_state(R, th, m, method, xi, si, times)
    u = (yT @ th['FL_w'].T + th['FL_b']).reshape(())
    a, b = torch.autograd.grad(u, [xi, si], create_graph=True, allow_unused=True)
    dv = b.reshape(()) * vs + (0.0 if a is None else (a.reshape(-1) * vx).sum())
    ut = (R.field(th, m, xi, times[-1], yT) @ th['FL_w'].T).reshape(())
    return _grads(u, th, retain_graph=True), _grads(dv, th, retain_graph=True), _grads(ut, th)


def forward_over_reverse(theta, m, method, x, s, times, vx, vs):
    """(Gu, Gd, Gt) with Gd as the tangent of (x, s) -> dU/dtheta along (vx, vs); Gu and Gt are plain gradients"""
    from oracle import refspec as R
    th = {k: theta[k].detach().clone().requires_grad_(True) for k in U_ORDER}

    def dU(xi, si):
        u = (_final_state(R, th, m, method, xi, si, times) @ th['FL_w'].T + th['FL_b']).reshape(())
        g = torch.autograd.grad(u, [th[k] for k in U_ORDER], create_graph=True, allow_unused=True)
        return tuple(torch.zeros_like(th[k]) if a is None else a for k, a in zip(U_ORDER, g))
    _, tan = torch.autograd.functional.jvp(dU, (x.detach().view(1, -1), s.detach().view(1)), (vx.view(1, -1), vs.view(1)))
    xi, si = x.detach().view(1, -1), s.detach().view(1)
    yT = _final_state(R, th, m, method, xi, si, times)
    u = (yT @ th['FL_w'].T + th['FL_b']).reshape(())
    ut = (R.field(th, m, xi, times[-1], yT) @ th['FL_w'].T).reshape(())
    return _grads(u, th, retain_graph=True), dict(zip(U_ORDER, (t.detach() for t in tan))), _grads(ut, th)


def flat(G):
    """a dict of gradients in theta's generic layout, flat [P_u]"""
    return torch.cat([G[k].reshape(-1) for k in U_ORDER])
