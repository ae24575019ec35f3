"""CPU restatement of solver 'explicit_adams' -- TEST INFRASTRUCTURE ONLY (the specification the HIP kernels
xw_adams_tiled_fwd_multi / xw_adams_tiled_bwd_multi of csrc/xw_tiled.hip are tested against).

The reference passes config['solver'] to torchdiffeq.odeint(..., method=...) (src/model.py:103-106).  'explicit_adams' is
torchdiffeq's fixed-grid Adams-Bashforth (fixed_adams.py: AdamsBashforth = AdamsBashforthMoulton with implicit=False).  The
package is absent from the reference tree and from this project, so this restates its published 0.1.x algorithm -- PARITY
UNPINNED, like oracle.refspec.odeint_fixed:
    on the requested grid t (cast to float64), for step n = 0 .. L-2: f_n = F(t_n, y_n) is pushed to the front of a history of
    at most _MAX_ORDER - 1 = 11 field values; order = min(len(history), 11); order < _MIN_ORDER - 1 = 3 (steps 0 and 1): one rk4
    step, 3/8 rule, with k1 = f_n (rk4_alt_step_func -- the project's rk4 tableau); otherwise
    y_{n+1} = y_n + sum_{j < order} (dt beta[order][j]) f_{n-j}, beta the order-step Adams-Bashforth row, most recent value first,
    applied at the current dt also on a non-uniform grid.  The outputs are the states at the grid points.
The coefficient rows are derived in exact rational arithmetic and converted to float64 once.
"""
from fractions import Fraction

import torch

F64 = torch.float64
MAX_ORDER, MIN_ORDER = 12, 4               # torchdiffeq fixed_adams.py _MAX_ORDER / _MIN_ORDER
HIST = MAX_ORDER - 1                       # the history's maxlen


def ab_row(k):
    """the k-step Adams-Bashforth row as Fractions, most recent value first: beta_j = integral over [0, 1] of the Lagrange basis
    polynomial of node -j among the nodes 0, -1, .., -(k-1) (time in steps, s = 0 at the current point)"""
    row = []
    for j in range(k):
        poly, den = [Fraction(1)], Fraction(1)            # coefficients, lowest power first
        for i in range(k):
            if i == j:
                continue
            poly = [i * poly[0]] + [poly[p - 1] + i * poly[p] for p in range(1, len(poly))] + [poly[-1]]   # * (s + i)
            den *= i - j
        row.append(sum(c / (p + 1) for p, c in enumerate(poly)) / den)
    return row


BASHFORTH = [None] + [ab_row(k) for k in range(1, HIST + 1)]          # BASHFORTH[k]: the k-step row (Fractions)
BASHFORTH64 = [None] + [[float(b) for b in row] for row in BASHFORTH[1:]]


def rk4_step(f, t0, dt, y, k1):
    """oracle.refspec.odeint_fixed's rk4 increment (the 3/8 rule) with a given k1"""
    k2 = f(t0 + dt / 3, y + dt * k1 / 3)
    k3 = f(t0 + 2 * dt / 3, y + dt * (k2 - k1 / 3))
    k4 = f(t0 + dt, y + dt * (k1 - k2 + k3))
    return dt * (k1 + 3 * (k2 + k3) + k4) / 8


def explicit_adams(f, y0, t, orders=None):
    """-> ys [N, L, ...] stacked along dim 1 like oracle.refspec.odeint_fixed.  `orders` (a list, optional) receives each step's
    order, 'rk4' for the start-up steps.  Autograd flows through every step (the grid is a constant)."""
    t = t.to(y0.dtype)
    ys, y, hist = [y0], y0, []
    for n in range(t.shape[0] - 1):
        t0, dt = t[n], t[n + 1] - t[n]
        fn = f(t0, y)
        hist = [fn] + hist[:HIST - 1]
        order = min(len(hist), HIST)
        if order < MIN_ORDER - 1:
            inc = rk4_step(f, t0, dt, y, fn)
            order = 'rk4'
        else:
            coef = dt * torch.tensor(BASHFORTH64[order], dtype=F64)
            inc = sum(coef[j] * hist[j] for j in range(order))
        y = y + inc
        ys.append(y)
        if orders is not None:
            orders.append(order)
    return torch.stack(ys, 1)


def odeint(f, y0, t, method):
    """oracle.refspec.odeint_fixed with 'explicit_adams' added (tests monkeypatch the oracle's integrator with this)"""
    if method == 'explicit_adams':
        return explicit_adams(f, y0, t)
    return ORIGINAL_ODEINT(f, y0, t, method)


def _original():
    from oracle import refspec as R
    return R.odeint_fixed


ORIGINAL_ODEINT = _original()


def u_net(theta, config, X, start_value):
    """oracle.refspec.u_net with solver 'explicit_adams' for a group that starts at T0 / on the boundary: u [N, L] (float64)"""
    from oracle import refspec as R
    m = config['u_layers']
    s = start_value.reshape(-1, 1).to(F64)
    y0 = torch.relu(torch.relu(s @ theta['IL0_w'].T + theta['IL0_b']) @ theta['IL2_w'].T + theta['IL2_b']) \
        @ theta['IL4_w'].T + theta['IL4_b']
    if X.shape[1] == 1:
        return y0 @ theta['FL_w'].T + theta['FL_b']
    x64 = X[:, 0, 1:].to(F64)
    ys = explicit_adams(lambda t, y: R.field(theta, m, x64, t, y), y0, X[0, :, 0])
    return (ys @ theta['FL_w'].T + theta['FL_b']).squeeze(2)
