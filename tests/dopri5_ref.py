"""CPU restatement of solver 'dopri5' -- TEST INFRASTRUCTURE ONLY (the specification the HIP kernels of csrc/xw_dopri.hip are
tested against).

The reference passes config['solver'] to torchdiffeq.odeint(..., method=...) with no rtol / atol / options
(src/model.py:103-106); 'dopri5' is torchdiffeq's default.  The package is absent from the reference tree and from this project,
so this is a restatement of its published 0.1.x algorithm -- PARITY UNPINNED, like oracle.refspec.odeint_fixed:
    Dormand-Prince 5(4) with FSAL; error ratio = RMS over the whole state of err / (atol + rtol max(|y0|, |y1|)); accept when
    ratio <= 1; next step dt min(ifactor, max(safety / ratio^(1/5), dfactor')) (dfactor' = 1 when ratio < 1; dt ifactor when
    ratio == 0); the first step by _select_initial_step (order 4); outputs from the quartic dense output of the first accepted
    step with t0 < t_i <= t1, steps never clipped to the output times.
`count`: the divisor of the RMS norms -- the NETWORK's N x u_hidden_dim (the kernels run narrower networks zero-padded).
`frozen`: a list of accepted (t0, dt) to integrate on instead of running the controller -- the grid as a constant, which is what
the kernels' backward pass differentiates.
"""
import math

import torch

F64 = torch.float64
RTOL, ATOL, SAFETY, IFACTOR, DFACTOR, ORDER = 1e-7, 1e-9, 0.9, 10.0, 0.2, 5

C = [0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0]
A = [[], [1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9], [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
     [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656], [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]]
B = [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0]
E = [35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720, -2187 / 6784 + 12231 / 42400,
     11 / 84 - 649 / 6300, -1 / 60]
MID = [6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
       187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2]


def rms(x, count=None):
    return torch.sqrt((x * x).sum() / (x.numel() if count is None else count))


def initial_step(f, t0, y0, f0, rtol, atol, count):
    """torchdiffeq _select_initial_step with order = 4 (dopri5's order - 1)"""
    scale = atol + torch.abs(y0) * rtol
    d0, d1 = rms(y0 / scale, count), rms(f0 / scale, count)
    h0 = torch.tensor(1e-6, dtype=F64) if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    f1 = f(t0 + h0, y0 + h0 * f0)
    d2 = rms((f1 - f0) / scale, count) / h0
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = torch.maximum(torch.tensor(1e-6, dtype=F64), h0 * 1e-3)
    else:
        h1 = (0.01 / torch.maximum(d1, d2)) ** (1.0 / 5)
    return torch.minimum(100 * h0, h1)


def rk_step(f, t0, dt, y0, f0):
    """one Dormand-Prince attempt: (y1, f1, error estimate, stages k_0..k_6)"""
    k = [f0]
    t1 = t0 + dt
    for s in range(1, 7):
        ys = y0 + sum(k[q] * (A[s][q] * dt) for q in range(s))
        k.append(f(t1 if s == 6 else t0 + C[s] * dt, ys))
    y1 = ys
    err = sum(k[q] * (dt * E[q]) for q in range(7))
    return y1, k[6], err, k


def interp_fit(y0, y1, y_mid, f0, f1, dt):
    """torchdiffeq _interp_fit: coefficients of the quartic in x = (t - t0) / (t1 - t0), lowest power first"""
    a = 2 * dt * (f1 - f0) - 8 * (y1 + y0) + 16 * y_mid
    b = dt * (5 * f0 - 3 * f1) + 18 * y0 + 14 * y1 - 32 * y_mid
    c = dt * (f1 - 4 * f0) - 11 * y0 - 5 * y1 + 16 * y_mid
    return [y0, dt * f0, c, b, a]


def interp_eval(coef, t0, t1, t):
    x = (t - t0) / (t1 - t0)
    return sum(cf * x ** i for i, cf in enumerate(coef))


def next_step(dt, ratio):
    """torchdiffeq _optimal_step_size, order 5"""
    if ratio == 0:
        return dt * IFACTOR
    dfac = 1.0 if ratio < 1 else DFACTOR
    return dt * torch.clamp(SAFETY / ratio ** (1.0 / ORDER), min=dfac, max=IFACTOR)


def dopri5(f, y0, t, rtol=RTOL, atol=ATOL, count=None, frozen=None, max_steps=10000):
    """-> (ys [N, L, ...] stacked along dim 1 like odeint_fixed, info dict(steps [(t0, dt)], n_att, n_acc, gap = min |ratio - 1|,
    cond = per attempt (condition number of the error ratio, whether the next step size moves with it)))
    t: float64 [L], increasing.  Autograd flows through the controller unless `frozen` is given."""
    t = t.to(F64)
    L = t.shape[0]
    f0 = f(t[0], y0)
    out = [y0] + [None] * (L - 1)
    i = 1
    while i < L and not bool(t[i] > t[0]):
        out[i] = y0
        i += 1
    steps, n_att, gap, cond = [], 0, math.inf, []
    t0, y = t[0], y0
    if frozen is None:
        dt = initial_step(f, t0, y0, f0, rtol, atol, count)
    it = iter(frozen or [])
    while i < L:
        if frozen is not None:
            t0f, dtf = next(it)
            t0, dt = torch.tensor(t0f, dtype=F64), torch.tensor(dtf, dtype=F64)
        assert bool(t0 + dt > t0), 'underflow in dt %r' % float(dt)
        y1, f1, err, k = rk_step(f, t0, dt, y, f0)
        n_att += 1
        if frozen is None:
            tol = atol + rtol * torch.maximum(y.abs(), y1.abs())
            ratio = rms(err / tol, count)
            gap = min(gap, abs(float(ratio.detach()) - 1.0))
            accept = bool(ratio <= 1)
            dt_next = next_step(dt, ratio)
            # the condition number of this attempt's ratio: the error estimate is a sum of seven terms that nearly cancel (the
            # weights E add up to zero), so one unit of relative rounding in the terms moves the ratio by `cond` units -- and,
            # where the step-size factor is not clamped, the next step size by cond / 5
            with torch.no_grad():
                mag = rms(sum(k[q].abs() * abs(float(dt) * E[q]) for q in range(7)) / tol, count)
                fac = float(dt_next / dt)
                free = float(ratio) > 0 and (1.0 if ratio < 1 else DFACTOR) < fac < IFACTOR
                cond.append((float(mag / ratio) if float(ratio) > 0 else math.inf, free))
        else:
            accept, dt_next = True, None
        if accept:
            t1 = t0 + dt
            y_mid = y + sum(k[q] * (dt * MID[q]) for q in range(7))
            coef = interp_fit(y, y1, y_mid, f0, f1, dt)
            while i < L and bool(t[i] <= t1):
                out[i] = interp_eval(coef, t0, t1, t[i])
                i += 1
            steps.append((float(t0.detach()), float(dt.detach())))
            if len(steps) >= max_steps and i < L:
                raise RuntimeError('step limit')
            t0, y, f0 = t1, y1, f1
        if frozen is None:
            dt = dt_next
    return torch.stack(out, 1), dict(steps=steps, n_att=n_att, n_acc=len(steps), gap=gap, cond=cond)


def u_net(theta, config, X, start_value, rtol=RTOL, atol=ATOL, frozen=None):
    """oracle.refspec.u_net with solver 'dopri5' for a group that starts at T0 / on the boundary: (u [N, L], info)"""
    from oracle import refspec as R
    m = config['u_layers']
    s = start_value.reshape(-1, 1).to(F64)
    y0 = torch.relu(torch.relu(s @ theta['IL0_w'].T + theta['IL0_b']) @ theta['IL2_w'].T + theta['IL2_b']) \
        @ theta['IL4_w'].T + theta['IL4_b']
    x64 = X[:, 0, 1:].to(F64)
    times = X[0, :, 0]
    ys, info = dopri5(lambda t, y: R.field(theta, m, x64, t, y), y0, times, rtol=rtol, atol=atol, count=y0.numel(),
                      frozen=frozen)
    return (ys @ theta['FL_w'].T + theta['FL_b']).squeeze(2), info
