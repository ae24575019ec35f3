"""tests/guarded.py on CPU tensors: the arena reports exactly what it claims to -- one changed guard element before or behind a
view, one output element that was not written, one overwritten element of a region stated as untouched -- and passes a clean
case; its views are what kernels._chk asks of an operand (dtype, contiguity, shape) at the stated alignment."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402

F64 = torch.float64


def _filled(arena):
    """an input, two outputs written in full, one output left alone"""
    a = arena.inp(torch.arange(37, dtype=F64).view(37, 1).expand(37, 3), name='x')
    u = arena.out(5, 37, name='u')
    y = arena.out(5, 7, 37, name='Y')
    gx = arena.out(3, 37, name='gx')
    u.copy_(torch.randn(5, 37, dtype=F64))
    y.copy_(torch.randn(5, 7, 37, dtype=F64))
    return a, u, y, gx


def test_a_clean_case_passes():
    arena = G.Arena('cpu')
    a, u, y, gx = _filled(arena)
    assert torch.equal(a, torch.arange(37, dtype=F64).view(37, 1).expand(37, 3))
    arena.check(written=[a, u, y], untouched=[gx])
    # a region: part of an output written, the rest stated as untouched -- as a slice and as a mask
    gx[:, :20] = 1.0
    mask = torch.zeros(3, 37, dtype=torch.bool)
    mask[:, 20:] = True
    arena.check(written=[u, y, gx[:, :20]], untouched=[gx[:, 20:], (gx, mask)])


@pytest.mark.parametrize('which', ['u', 'Y', 'x'])
@pytest.mark.parametrize('side', ['before', 'behind'])
def test_one_changed_guard_element_is_reported(which, side):
    arena = G.Arena('cpu')
    a, u, y, gx = _filled(arena)
    t = {'u': u, 'Y': y, 'x': a}[which]
    c, e, name = arena._where(t)
    at = e - 1 if side == 'before' else e + t.numel()
    assert bool(c.guard[at])
    c.f64[at] = 0.0                                             # a store of a plausible number, one double outside the view
    with pytest.raises(AssertionError, match='guard band overwritten.*1 doubles %s the %s of %s' % (
            side, 'start' if side == 'before' else 'end', name)):
        arena.check(written=[a, u, y], untouched=[gx])


def test_a_guard_element_rewritten_with_another_nan_is_reported():
    """compared as int64: a NaN of another bit pattern is a store too"""
    arena = G.Arena('cpu')
    a, u, y, gx = _filled(arena)
    c, e, _ = arena._where(y)
    c.f64[e + y.numel() + G.GUARD - 1] = float('nan')
    assert c.raw[e + y.numel() + G.GUARD - 1] != G.PATTERN
    with pytest.raises(AssertionError, match='guard band overwritten'):
        arena.check(written=[a, u, y], untouched=[gx])


def test_one_unwritten_output_element_is_reported():
    arena = G.Arena('cpu')
    a, u, y, gx = _filled(arena)
    y[3, 6, 36] = arena.out(1)[0]                               # (the pattern: as if the kernel had skipped the last path)
    with pytest.raises(AssertionError, match=r'Y#\d+: element \(3, 6, 36\) was not written'):
        arena.check(written=[a, u, y], untouched=[gx])


def test_one_overwritten_untouched_element_is_reported():
    arena = G.Arena('cpu')
    a, u, y, gx = _filled(arena)
    gx[2, 5] = 0.0
    with pytest.raises(AssertionError, match=r'gx#\d+: element \(2, 5\) of a region the kernels leave untouched'):
        arena.check(written=[a, u, y], untouched=[gx])
    mask = torch.zeros(3, 37, dtype=torch.bool)
    mask[2, 5] = True
    with pytest.raises(AssertionError, match=r'gx#\d+: element \(2, 5\)'):
        arena.check(untouched=[(gx, mask)])
    arena.check(untouched=[(gx, ~mask)])                        # (the other elements are still the pattern)


def test_views_are_operands_the_wrappers_accept():
    """what kernels._chk asks of an operand besides its device -- float64, contiguous, the requested shape -- asserted directly,
    ALIGN-byte alignment, GUARD doubles of pattern on both sides, also across a buffer that fills up.  (_chk itself stops at its
    first test on a CPU tensor, the device: the GPU cases pass every view through it.)"""
    from xnode_wan_pde_solver_amd import kernels as KN
    from xnode_wan_pde_solver_amd._lib import XnwanError
    arena = G.Arena('cpu', chunk=4096)
    shapes = [(1,), (3, 5), (2, 7, 33), (4000,), (17,), (9, 255), (1, 1)]
    views = [arena.out(*s) for s in shapes] + [arena.inp(torch.randn(31, 2, dtype=F64))]
    assert len(arena.chunks) > 1                                # (the requests did not fit one buffer)
    for v, s in zip(views, shapes + [(31, 2)]):
        assert v.dtype == F64 and v.is_contiguous() and tuple(v.shape) == s and v.data_ptr() % G.ALIGN == 0
        c, e, _ = arena._where(v)
        assert bool(c.guard[e - G.GUARD:e].all()) and bool(c.guard[e + v.numel():e + v.numel() + G.GUARD].all())
        assert bool((c.raw[e - G.GUARD:e] == G.PATTERN).all()) and bool((c.raw[e + v.numel():e + v.numel() + G.GUARD] == G.PATTERN).all())
        with pytest.raises(XnwanError, match='must be a CUDA/HIP tensor'):
            KN._chk(v, F64, s, 'view')
    for v in views[:-1]:
        assert bool(torch.isnan(v).all()) and bool((v.view(torch.int64) == G.PATTERN).all())
    arena.check(untouched=views[:-1], written=views[-1:])


def test_workspace_patch_hands_out_guarded_views_of_the_same_size():
    class KN:                                                   # (a stand-in for the kernels module: two allocators)
        @staticmethod
        def tiled_ode_work(sweep, d, H, K, m, tiles, dev, method=None):
            return torch.empty(100 * tiles + (7 if sweep else 3), dtype=F64, device=dev)

        @staticmethod
        def _dopri5_tiled_work(sweep, d, H, K, m, Ns, dev):
            return torch.empty(11 * sum((N + 15) // 16 for N in Ns), dtype=F64, device=dev)

    orig = KN.tiled_ode_work
    arena = G.Arena('cpu')
    with arena.workspaces(KN):
        w1 = KN.tiled_ode_work(True, 3, 20, 10, 2, 4, 'cpu', method=None)
        w2 = KN._dopri5_tiled_work(False, 3, 20, 10, 2, [1, 17, 33], 'cpu')
        assert w1.shape == (407,) and w2.shape == (11 * 6,)
        assert bool((w1.view(torch.int64) == G.PATTERN).all()) and bool((w2.view(torch.int64) == G.PATTERN).all())
    assert KN.tiled_ode_work is orig                            # (restored on exit)
    w1[:] = 1.0                                                 # a workspace is the kernels' to write ...
    arena.check()
    c, e, _ = arena._where(w1)
    c.f64[e + 407] = 1.0                                        # ... but not past its end
    with pytest.raises(AssertionError, match='1 doubles behind the end of tiled_ode_work'):
        arena.check()


def test_record_patch_keeps_the_dopri5_record_in_the_arena():
    class KN:                                                   # (a stand-in for the kernels module: the record class alone)
        class Dopri5Record:
            def __init__(self, N, H, cap, dev, stepper='vector'):
                self.N, self.H, self.cap = N, H, cap
                self.rec_y = torch.empty(cap + 1, H, N, dtype=F64, device=dev)
                self.rec_t = torch.empty(cap + 1, dtype=F64, device=dev)
                self.rec_h = torch.empty(max(cap, 1), dtype=F64, device=dev)
                self.fbuf = torch.empty(2, H, N, dtype=F64, device=dev)
                self.work = torch.empty(2 * ((N + 63) // 64), dtype=F64, device=dev)

            def grow(self, cap, n_acc):
                y, tt, h = self.rec_y, self.rec_t, self.rec_h
                self.rec_y = torch.empty(cap + 1, self.H, self.N, dtype=F64, device=y.device)
                self.rec_t = torch.empty(cap + 1, dtype=F64, device=y.device)
                self.rec_h = torch.empty(cap, dtype=F64, device=y.device)
                self.rec_y[:n_acc + 1].copy_(y[:n_acc + 1])
                self.rec_t[:n_acc + 1].copy_(tt[:n_acc + 1])
                self.rec_h[:n_acc].copy_(h[:n_acc])
                self.cap = cap

    orig = KN.Dopri5Record
    arena = G.Arena('cpu')
    with arena.dopri5_records(KN):
        r = KN.Dopri5Record(65, 3, 2, 'cpu')
        assert isinstance(r, orig)
        first = {k: getattr(r, k) for k in ('rec_y', 'rec_t', 'rec_h', 'fbuf', 'work')}
        assert {k: tuple(v.shape) for k, v in first.items()} == {'rec_y': (3, 3, 65), 'rec_t': (3,), 'rec_h': (2,), 'fbuf': (2, 3, 65),
                                                                 'work': (4,)}
        for v in first.values():
            arena._where(v)                                     # (a view of this arena)
            assert bool((v.view(torch.int64) == G.PATTERN).all())
        r.rec_y[:2] = 1.0                                       # one accepted step, as the kernels would leave it
        r.rec_t[:2] = torch.tensor([0.0, 0.5], dtype=F64)
        r.rec_h[:1] = 0.5
        r.grow(5, 1)
        assert r.cap == 5 and tuple(r.rec_y.shape) == (6, 3, 65) and tuple(r.rec_t.shape) == (6,) and tuple(r.rec_h.shape) == (5,)
        assert r.fbuf is first['fbuf'] and r.work is first['work'] and r.rec_y is not first['rec_y']
        assert float(r.rec_y[:2].min()) == 1.0 and r.rec_t[:2].tolist() == [0.0, 0.5] and r.rec_h[:1].tolist() == [0.5]
    assert KN.Dopri5Record is orig                              # (restored on exit)
    arena.check(written=[r.rec_y[:2], r.rec_t[:2], r.rec_h[:1], first['rec_y'][:2]],
                untouched=[r.rec_y[2:], r.rec_t[2:], r.rec_h[1:], r.fbuf, r.work, first['rec_y'][2:]])
    c, e, _ = arena._where(first['rec_y'])                      # a store behind the end of the record that was replaced
    c.f64[e + first['rec_y'].numel()] = 1.0
    with pytest.raises(AssertionError, match=r'1 doubles behind the end of dopri5\.rec_y#'):
        arena.check()
    c.raw[e + first['rec_y'].numel()] = G.PATTERN
    c, e, _ = arena._where(r.rec_h)                             # ... and one behind the grown step-size record
    c.f64[e + 5] = 0.25
    with pytest.raises(AssertionError, match=r'1 doubles behind the end of dopri5\.rec_h\(cap 5\)'):
        arena.check()
