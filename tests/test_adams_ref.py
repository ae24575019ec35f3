"""Solver 'explicit_adams' on the host: the CPU restatement (tests/adams_ref.py) pinned against the method's definition, the
coefficients the kernels use, and the host logic that routes the solver to the tiled stepper family.  No kernel is launched."""
import ctypes
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adams_ref as A  # noqa: E402

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAMS_NAMES = ('xw_adams_coef', 'xw_adams_tiled_work', 'xw_adams_tiled_fwd_multi', 'xw_adams_tiled_bwd_multi')


# ---- the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(1, A.HIST + 1))
def test_each_row_sums_to_one_and_integrates_every_polynomial_of_degree_below_k(k):
    """sum_j beta_j (-j)^q = integral_0^1 s^q ds for q < k, exactly: one AB_k step is exact on y' = p(t), deg p <= k - 1, on a
    uniform grid -- k conditions for the k unknowns, so this pins the row"""
    row = A.BASHFORTH[k]
    assert len(row) == k and sum(row) == 1
    for q in range(k):
        assert sum(b * Fraction(-j) ** q for j, b in enumerate(row)) == Fraction(1, q + 1), (k, q)
    assert A.BASHFORTH64[k] == [float(b) for b in row]


def test_known_rows():
    assert A.BASHFORTH[3] == [Fraction(23, 12), Fraction(-16, 12), Fraction(5, 12)]
    assert A.BASHFORTH[4] == [Fraction(55, 24), Fraction(-59, 24), Fraction(37, 24), Fraction(-9, 24)]
    assert [b * 720 for b in A.BASHFORTH[5]] == [1901, -2774, 2616, -1274, 251]


def test_one_step_is_exact_on_polynomials_in_floating_point():
    """the restatement's steps n >= 2 on y' = p(t) (deg p = order - 1, uniform grid): y_{n+1} - y_n is the integral of p to rounding"""
    g = torch.Generator().manual_seed(1)
    L, h = 14, 0.05
    t = 0.3 + h * torch.arange(L, dtype=F64)
    orders = []
    A.explicit_adams(lambda tt, y: torch.zeros_like(y), torch.zeros(1, 1, dtype=F64), t, orders)
    for n, order in enumerate(orders):
        if order == 'rk4':
            continue
        c = torch.randn(order, dtype=F64, generator=g)               # p(t) = sum_q c_q t^q, degree order - 1
        ys = A.explicit_adams(lambda tt, y: sum(c[q] * tt ** q for q in range(order)) * torch.ones_like(y), torch.zeros(1, 1, dtype=F64), t)
        exact = sum(c[q] * (t[n + 1] ** (q + 1) - t[n] ** (q + 1)) / (q + 1) for q in range(order))
        got = ys[0, n + 1, 0] - ys[0, n, 0]
        assert abs(float(got - exact)) <= 1e-13 * max(1.0, abs(float(exact))), (n, order)


def _field(seed=0):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(5, 5, dtype=F64, generator=g) * 0.5
    b = torch.randn(5, dtype=F64, generator=g)
    return lambda t, y: torch.tanh(y @ W.T + b * t) - 0.3 * y


def test_start_up_steps_are_the_projects_rk4_step():
    from oracle import refspec as R
    f = _field()
    y0 = torch.randn(4, 5, dtype=F64, generator=torch.Generator().manual_seed(2))
    t = torch.tensor([0.1, 0.25, 0.32], dtype=F64)
    assert torch.equal(A.explicit_adams(f, y0, t), R.odeint_fixed(f, y0, t, 'rk4'))
    assert torch.equal(A.explicit_adams(f, y0, t[:2]), R.odeint_fixed(f, y0, t[:2], 'rk4'))


@pytest.mark.parametrize('L', [1, 2, 3, 4, 13, 32])
def test_order_sequence_and_short_grids(L):
    f = _field(3)
    y0 = torch.randn(2, 5, dtype=F64, generator=torch.Generator().manual_seed(4))
    t = torch.linspace(0, 0.4, L, dtype=F64) if L > 1 else torch.tensor([0.2], dtype=F64)
    orders = []
    ys = A.explicit_adams(f, y0, t, orders)
    assert ys.shape == (2, L, 5) and torch.equal(ys[:, 0], y0)
    want = (['rk4', 'rk4'] + list(range(3, A.HIST + 1)) + [A.HIST] * L)[:max(L - 1, 0)]
    assert orders == want
    if L == 13:
        assert orders[2:] == [3, 4, 5, 6, 7, 8, 9, 10, 11, 11]


def test_fourth_order_convergence_on_exponential_decay():
    """y' = -y on [0, 0.1]: halving the step shrinks the error at the end by the 4th-order factor or more (the AB3 step's local
    error leads; on longer intervals the high-order rows' small stability intervals show instead: DESIGN section 8)"""
    errs = []
    for N in (8, 16):
        t = torch.linspace(0, 0.1, N + 1, dtype=F64)
        ys = A.explicit_adams(lambda tt, y: -y, torch.ones(1, 1, dtype=F64), t)
        errs.append(abs(float(ys[0, -1, 0]) - math.exp(-0.1)))
    assert errs[0] / errs[1] >= 15.0, errs


def test_non_uniform_grid_uses_the_fixed_coefficients():
    """on a non-uniform grid every AB step applies the uniform-grid row at its own dt (torchdiffeq's behaviour), so a polynomial
    the row integrates exactly on a uniform grid is NOT integrated exactly"""
    t = torch.tensor([0.0, 0.1, 0.15, 0.3, 0.34, 0.5, 0.55], dtype=F64)
    p = lambda tt: 1 + tt + tt ** 2                                   # noqa: E731
    ys = A.explicit_adams(lambda tt, y: p(tt) * torch.ones_like(y), torch.zeros(1, 1, dtype=F64), t)
    for n in range(2, 6):
        order = min(n + 1, A.HIST)
        dt = t[n + 1] - t[n]
        want = sum((dt * A.BASHFORTH64[order][j]) * p(t[n - j]) for j in range(order))
        assert abs(float(ys[0, n + 1, 0] - ys[0, n, 0] - want)) < 1e-15
    exact = lambda a, b: (b - a) + (b ** 2 - a ** 2) / 2 + (b ** 3 - a ** 3) / 3   # noqa: E731
    assert abs(float(ys[0, 3, 0] - ys[0, 2, 0] - exact(t[2], t[3]))) > 1e-4


# ---- the coefficients the kernels use and the C ABI ------------------------------------------------------------------------
def test_kernel_coefficients_are_the_rational_rows_rounded_once():
    from xnode_wan_pde_solver_amd import _lib
    buf = (ctypes.c_double * A.HIST)()
    for k in range(1, A.HIST + 1):
        assert _lib.lib.xw_adams_coef(k, ctypes.cast(buf, ctypes.c_void_p)) == 0
        assert list(buf)[:k] == A.BASHFORTH64[k], k                 # bit for bit
    assert _lib.lib.xw_adams_coef(0, ctypes.cast(buf, ctypes.c_void_p)) == -2
    assert _lib.lib.xw_adams_coef(12, ctypes.cast(buf, ctypes.c_void_p)) == -2


def test_adams_symbols_are_declared_exported_and_mirrored():
    from xnode_wan_pde_solver_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'xnwan.h')).read()
    assert set(re.findall(r'^\s*int\s+(xw_adams_\w+)\s*\(', hdr, flags=re.M)) == set(ADAMS_NAMES)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(ADAMS_NAMES) <= set(re.findall(r'\bT\s+(xw_\w+)', out))
    for name in ADAMS_NAMES:
        args = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')
        assert len(args) == len(_lib.SIGNATURES[name]), name
    assert _lib.ABI_VERSION == 33 == _lib.lib.xw_abi_version()


def test_adams_workspace_is_the_tiled_one_plus_the_history():
    from xnode_wan_pde_solver_amd import _lib
    for H, K, m in ((20, 10, 8), (128, 64, 8), (256, 256, 32)):
        assert _lib.lib.xw_adams_tiled_work(0, 20, H, K, m) == _lib.lib.xw_tiled_ode_work(0, 20, H, K, m) + 16 * H * 11
        assert _lib.lib.xw_adams_tiled_work(1, 20, H, K, m) == _lib.lib.xw_tiled_ode_work(1, 20, H, K, m) + 16 * H * 12
    assert _lib.lib.xw_adams_tiled_work(0, 20, 257, 16, 8) == -1


def test_c_abi_refusals_before_any_launch():
    """the adams sweep refuses the adjoint / narrow mode bits; the fixed-grid tiled, fused and generic entry points refuse the
    explicit_adams id (4) with XW_E_ARG -- all before any job is read"""
    from xnode_wan_pde_solver_amd import _lib
    L_ = _lib.lib
    dummy = ctypes.c_void_p(16)                                      # (never dereferenced: the refusal comes first)
    bj = (_lib.XwOdeBwdJob * 1)()
    bj[0].N = 16
    fj = (_lib.XwOdeFwdJob * 1)()
    assert L_.xw_adams_tiled_bwd_multi(bj, 1, dummy, dummy, 4, 5, 20, 10, 8, 8 | 3, dummy, None) == -1
    assert L_.xw_adams_tiled_bwd_multi(bj, 1, dummy, dummy, 4, 5, 20, 10, 8, 16 | 3, dummy, None) == -1
    assert L_.xw_adams_tiled_bwd_multi(bj, 1, dummy, dummy, 4, 5, 20, 10, 8, 0, dummy, None) == -2
    assert L_.xw_adams_tiled_fwd_multi(fj, 1, dummy, dummy, 4, 5, 257, 10, 8, None, dummy, None) == -1
    assert L_.xw_adams_tiled_fwd_multi(fj, 1, dummy, dummy, 0, 5, 20, 10, 8, None, dummy, None) == -2      # L = 0
    assert L_.xw_tiled_ode_fwd_multi(fj, 1, dummy, dummy, 4, 4, 5, 128, 32, 8, None, dummy, None) == -2
    assert L_.xw_tiled_ode_bwd_multi(bj, 1, dummy, dummy, 4, 4, 5, 128, 32, 8, 3, dummy, None) == -2
    for H, K, m in ((20, 10, 8), (64, 16, 8), (48, 16, 11)):                 # fused containers and the generic path
        assert L_.xw_ode_fwd_multi(fj, 1, dummy, dummy, 4, 4, 5, H, K, m, None, None) == -2, (H, K, m)
        assert L_.xw_ode_bwd_multi(bj, 1, dummy, dummy, 4, 4, 5, H, K, m, 3, None) == -2, (H, K, m)


# ---- host logic ----------------------------------------------------------------------------------------------------------
def test_method_id_serves_explicit_adams_and_refuses_the_rest():
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    assert KN.method_id('explicit_adams') == KN.ADAMS == 4
    assert KN.ADAMS not in KN.METHODS.values() and KN.METHODS == {'euler': 0, 'midpoint': 1, 'rk4': 2}
    assert KN.method_id('dopri5') == KN.DOPRI5
    for name in ('implicit_adams', 'fixed_adams', 'adams', 'dopri8', 'bosh3', 'adaptive_heun', 'fehlberg2', 'nonsense'):
        with pytest.raises(XnwanError, match='dopri5') as e:
            KN.method_id(name)
        assert 'explicit_adams' in str(e.value)


@pytest.mark.parametrize('H,K,m', [(20, 10, 8), (30, 10, 8), (64, 16, 12), (128, 64, 8), (256, 256, 32), (1, 1, 1)])
def test_explicit_adams_takes_the_tiled_family_at_every_width(H, K, m):
    from xnode_wan_pde_solver_amd import kernels as KN
    assert KN.stepper_family(H, K, m, method=KN.ADAMS) == 'tiled'
    assert KN.stepper_family(H, K, m, 'generic', KN.ADAMS) == 'tiled'
    assert KN.stepper_kdims(H, K, m, method=KN.ADAMS) == (H, K)
    for mid in (None, 0, 1, 2, KN.DOPRI5):                              # every other method: unchanged
        assert KN.stepper_family(H, K, m, method=mid) == KN.stepper_family(H, K, m)
        assert KN.stepper_kdims(H, K, m, method=mid) == KN.stepper_kdims(H, K, m)


def test_explicit_adams_beyond_the_tiled_limits_raises():
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    with pytest.raises(XnwanError, match='256'):
        KN.stepper_family(257, 16, 8, method=KN.ADAMS)


def test_xnode_binds_at_its_own_widths_and_refuses_the_adjoint():
    from xnode_wan_pde_solver_amd import kernels as KN, nets
    from xnode_wan_pde_solver_amd._lib import XnwanError
    net = nets.XNODE(30, 1, None, None, {'dim': 4}, 10, 8, None, solver='explicit_adams')
    blob = net.bind(torch.device('cpu'))
    assert net.method == KN.ADAMS and net.family == 'tiled' and net.kdims == (30, 10)   # (midpoint: the (32, 12) container)
    assert blob.data.numel() == KN.theta_size(4, 30, 10) == sum(p.numel() for p in net.parameters())
    with pytest.raises(XnwanError, match="'explicit_adams' with adjoint=True"):
        nets.XNODE(20, 1, None, None, {'dim': 4}, 10, 8, None, solver='explicit_adams', adjoint=True)
