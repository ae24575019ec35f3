"""CPU-side checks of the evaluation at scattered points (xnode_wan_pde_solver_amd/evalpaths.py, csrc/xw_tiled_paths.hip): the
per-point grids and their packing against a brute-force loop, the domains' entry rules against func_w, the sort, the new C-ABI
symbols and every refusal.  No kernel is launched."""
import math
import os
import re
import subprocess

import pytest
import torch

from xnode_wan_pde_solver_amd import evalpaths as EP, kernels as KN, sampling, _lib
from xnode_wan_pde_solver_amd.options import EngineOptions
from xnode_wan_pde_solver_amd._lib import XnwanError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


# ---- grids ---------------------------------------------------------------------------------------------------------------------------
def _brute(t, t_in, T0, T, n_sub):
    """one point, Python floats: (n, [grid])"""
    step = (T - T0) / n_sub
    n = 0 if t == t_in else max(1, math.ceil((t - t_in) / step))
    return n, [t_in + (t - t_in) * k / n for k in range(n)] + [t]


def _points(dtype):
    g = torch.Generator().manual_seed(3)
    T0, T, n_sub = 0.0, 1.0, 8
    step = (T - T0) / n_sub
    t = torch.rand(40, generator=g, dtype=F64)
    t[0], t[1], t[2] = T0, T, 3 * step                          # t == t_in, the whole interval, an exact multiple of the step
    t[3] = math.nextafter(3 * step, 2.0)                        # one ulp above a multiple: one more step
    t[4] = math.nextafter(3 * step, 0.0)
    t[5] = math.nextafter(0.0, 1.0)                             # the smallest positive time: one step
    t_in = torch.zeros(40, dtype=F64)
    t_in[20:] = t[20:] * torch.rand(20, generator=g, dtype=F64)    # late entries
    t_in[20] = t[20]                                            # ... one of them with t == t_in
    t = t.to(dtype).to(F64)                                     # (float32 input: widened exactly, then everything in float64)
    t_in = torch.minimum(t_in.to(dtype).to(F64), t)
    return t, t_in, T0, T, n_sub


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_grids_match_a_brute_force_loop(dtype):
    t, t_in, T0, T, n_sub = _points(dtype)
    n = EP.step_counts(t, t_in, T0, T, n_sub)
    tT = EP.pack_grids(t, t_in, n)
    want = [_brute(float(a), float(b), T0, T, n_sub) for a, b in zip(t, t_in)]
    assert n.tolist() == [w[0] for w in want]
    assert n[0] == 0 and n[20] == 0 and n[1] == n_sub and n[2] == 3 and n[4] == 3
    if dtype == torch.float64:                                  # (in float32 the three neighbours of 3 steps are one number)
        assert n[3] == 4 and n[5] == 1                          # one ulp above 3 steps: a fourth; the smallest time: one
    L = max(w[0] for w in want) + 1
    assert tT.shape == (L, 40) and tT.dtype == F64 and tT.is_contiguous()
    for i, (ni, grid) in enumerate(want):
        col = tT[:, i].tolist()
        assert col[:ni + 1] == grid, i                          # the same bits as the loop
        assert all(v == float(t[i]) for v in col[ni:]), i       # ends exactly at t; the padding repeats it
    assert bool((tT[1:] >= tT[:-1]).all())
    assert torch.equal(EP.last_distinct(tT), n.to(torch.int32))


def test_last_distinct_of_a_general_group():
    tT = torch.tensor([[0.0, 0.0, 0.5], [0.0, 0.25, 0.5], [1.0, 0.25, 0.5], [1.0, 0.75, 0.5]], dtype=F64)
    assert EP.last_distinct(tT).tolist() == [2, 3, 0]
    assert EP.last_distinct(tT[:1]).tolist() == [0, 0, 0]


def test_sort_and_unsort_is_a_permutation():
    g = torch.Generator().manual_seed(5)
    n = torch.randint(0, 9, (101,), generator=g)
    order, inverse = EP.sort_by_steps(n)
    assert sorted(order.tolist()) == list(range(101)) and sorted(inverse.tolist()) == list(range(101))
    assert bool((n[order][1:] >= n[order][:-1]).all())
    vals = torch.randn(101, generator=g)
    assert torch.equal(vals[order][inverse], vals)
    # stable: equal step counts keep their order
    assert all(a < b for a, b in zip(order.tolist(), order.tolist()[1:]) if n[a] == n[b])


# ---- entry rules -----------------------------------------------------------------------------------------------------------------------
def _ball_points(r, d, seed, M=200):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, d, generator=g, dtype=F64)
    x = r * z / z.norm(dim=1, keepdim=True) * torch.rand(M, 1, generator=g, dtype=F64) ** (1 / d)
    return torch.cat((torch.rand(M, 1, generator=g, dtype=F64), x), 1)


def test_cube_and_cone_enter_at_T0():
    pts = _ball_points(1.0, 3, 1)
    for cls, sp in ((sampling.Hypercube, [-1, 1]), (sampling.NSphere_TCone, 1.0)):
        t_in, at_T0 = cls.entry(pts, sp, 0, 1)
        assert t_in.dtype == F64 and torch.equal(t_in, torch.zeros(200, dtype=F64)) and bool(at_T0.all())
        t_in, _ = cls.entry(pts, sp, 0.25, 1)
        assert torch.equal(t_in, torch.full((200,), 0.25, dtype=F64))


def test_hourglass_entry_is_bound_pads_rule_per_point():
    r, T0, T = 1.5, 0, 1
    pts = _ball_points(r, 3, 2)
    half = (T - T0) / 2
    t_in, at_T0 = sampling.NSphere_THourglass.entry(pts, r, T0, T)
    rad = pts[:, 1:].norm(dim=1)
    early, inner = pts[:, 0] < half, rad <= r * half
    assert torch.equal(at_T0, early | inner)
    assert 0 < int((~at_T0).sum()) < 200 and int(early.sum()) > 0 and int((~early & inner).sum()) > 0
    assert bool((t_in[at_T0] == T0).all())
    # points that left the inner ball: the entry point lies on the moving boundary (func_w = 0), in the widening half
    dom = sampling.NSphere_THourglass.__new__(sampling.NSphere_THourglass)     # (no __init__: a domain object draws a time grid)
    dom.r, dom.T0, dom.T, dom.N_t = r, T0, T, 4
    first = torch.cat((t_in.view(-1, 1), pts[:, 1:]), 1)[~at_T0]
    assert float(dom.func_w(first.unsqueeze(1)).abs().max()) < 1e-12
    assert bool((first[:, 0] > half).all())
    # bound_pad, one path at a time, starts its grid at the same entry time (points inside the domain: t >= t_in)
    inside = (pts[:, 0] >= t_in).nonzero().view(-1).tolist()
    kinds = {(bool(early[k]), bool(inner[k])) for k in inside}
    assert {(True, True), (True, False), (False, True), (False, False)} <= kinds
    for k in inside[:60]:
        _, _, grids = dom.bound_pad(pts[k].view(1, 1, -1).repeat(2, 1, 1))       # (twice: bound_pad squeezes its per-path flags)
        assert float(grids[0][0]) == float(t_in[k]), k


def test_entry_draws_no_random_numbers():
    pts = _ball_points(1.0, 3, 4)                               # (a generator of its own)
    st = torch.get_rng_state()
    for cls, sp in ((sampling.Hypercube, [-1, 1]), (sampling.NSphere_TCone, 1.0), (sampling.NSphere_THourglass, 1.0)):
        cls.entry(pts, sp, 0, 1)
    assert torch.equal(torch.get_rng_state(), st)


# ---- symbols ---------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'xnwan.h')).read()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ('xw_paths_tiled_fwd', 'xw_paths_tiled_work'):
        args = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')
        assert len(args) == len(_lib.SIGNATURES[name]), name
        assert re.search(r'\bT\s+' + name + r'\b', out), name
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name]
    body = re.search(r'typedef struct \{([^}]*)\}\s*XwPathsJob\s*;', hdr).group(1)
    fields = [re.split(r'[\s\*]+', decl.strip())[-1] for decl in body.split(';') if decl.strip()]
    assert fields == [f[0] for f in _lib.XwPathsJob._fields_] == ['xT', 'start', 'tT', 'nstep', 'u', 'Y', 'N', 'last_only']
    assert _lib.ABI_VERSION == 33 == _lib.lib.xw_abi_version()
    # the kernel is in the library's gfx950 code object
    blob = open(_lib.LIB_PATH, 'rb').read()
    assert b'kt_ode_fwd_pp' in blob
    assert callable(KN.tiled_paths_fwd) and EngineOptions().eval_chunk_paths == 65536 == EP.EVAL_CHUNK_PATHS


def test_workspace_query_and_host_side_refusals_of_the_entry_point():
    lib = _lib.lib
    for dims in ((20, 20, 10, 8), (3, 65, 16, 1), (5, 256, 256, 32)):
        assert lib.xw_paths_tiled_work(*dims) == lib.xw_tiled_ode_work(0, *dims) > 0
    assert lib.xw_paths_tiled_work(20, 257, 16, 8) == -1
    job = (_lib.XwPathsJob * 1)()
    job[0].xT = job[0].start = job[0].tT = job[0].u = 8            # (never dereferenced: every call below is refused on the host)
    job[0].N = 1
    call = lambda method, H, njobs=1: lib.xw_paths_tiled_fwd(job, njobs, 8, method, 2, 3, H, 10, 8, 8, None)   # noqa: E731
    assert call(3, 20) == -2 and call(4, 20) == -2 and call(-1, 20) == -2          # XW_E_ARG: method ids other than 0, 1, 2
    assert call(0, 257) == -1                                                      # XW_E_DIMS where xw_tiled_ode_ok is 0
    assert call(0, 20, njobs=0) == -2
    job[0].tT = None
    assert call(0, 20) == -2


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
SETUP = {'dim': 3, 'N_t': 4, 'T0': 0, 'T': 1, 'shape_param': 1.0}


def _evaluate(points, solver='midpoint', domain=sampling.NSphere_THourglass, n_sub=None, setup=SETUP):
    h = lambda X0: X0[:, 1]              # noqa: E731
    g = lambda BX: BX[..., 1]            # noqa: E731
    return EP.evaluate_points(points, n_sub, setup, domain, solver, h, g, torch.zeros(1, dtype=F64), KN.method_id(solver), 20, 10, 8,
                              torch.device('cpu'))


@pytest.mark.parametrize('solver', ['dopri5', 'explicit_adams'])
def test_evaluate_refuses_the_solvers_without_a_per_path_form(solver):
    with pytest.raises(XnwanError, match=solver):
        _evaluate(torch.zeros(2, 4, dtype=F64), solver=solver)
    with pytest.raises(XnwanError, match='fixed-grid'):
        _evaluate(torch.zeros(2, 4), solver=solver)


def test_evaluate_refuses_points_before_their_entry_time():
    # the widening half, outside the inner ball: entered at |x| / r = 0.8; t = 0.7 lies before it
    pts = torch.tensor([[0.7, 0.8, 0.0, 0.0], [0.9, 0.8, 0.0, 0.0]], dtype=F64)
    with pytest.raises(XnwanError, match='t >= t_in') as e:
        _evaluate(pts)
    assert '1 points' in str(e.value) and 'point 0' in str(e.value)
    with pytest.raises(XnwanError, match='t >= t_in'):
        _evaluate(torch.tensor([[0.1, 0.0, 0.0, 0.0]], dtype=F64), domain=sampling.Hypercube,
                  setup=dict(SETUP, T0=0.25, shape_param=[-1, 1]))


def test_evaluate_refuses_a_domain_class_without_entry():
    class Slab:
        pass
    with pytest.raises(XnwanError, match='Slab.*entry'):
        _evaluate(torch.zeros(2, 4, dtype=F64), domain=Slab)
    with pytest.raises(XnwanError, match='Slab.*entry'):
        _evaluate(torch.zeros(2, 4, dtype=F64), domain=Slab())


def test_evaluate_refuses_bad_shapes_and_resolutions():
    with pytest.raises(XnwanError, match=r'\[M, 4\]'):
        _evaluate(torch.zeros(2, 5, dtype=F64))
    with pytest.raises(XnwanError, match='n_sub'):
        _evaluate(torch.zeros(2, 4, dtype=F64), n_sub=0)
    with pytest.raises(XnwanError, match='eval_chunk_paths'):
        EP.paths_forward(torch.zeros(3, 2, dtype=F64), torch.zeros(1, 2, dtype=F64), torch.zeros(2, dtype=F64), None,
                         torch.zeros(1, dtype=F64), 0, 20, 10, 8, chunk=0)


def test_public_surface_exists():
    from xnode_wan_pde_solver_amd import nets, solver, engine
    assert callable(nets.XNODE.evaluate) and callable(solver.NODE_WAN_solver.evaluate) and callable(engine.Engine.predict_paths)
    for cls in sampling.DOMAINS.values():
        assert callable(cls.entry)
