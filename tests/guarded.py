"""Guard-banded, poisoned buffers for kernel tests -- TEST INFRASTRUCTURE ONLY (imported like tests/adams_ref.py).

Arena(device) hands out contiguous float64 tensors that are views into one larger buffer (a further one is opened when it is
full).  Every element of that buffer that no view owns is a GUARD: it holds one fixed quiet-NaN bit pattern (PATTERN), at least
GUARD doubles before and behind every view, and check() compares all of them bit for bit -- a store a few doubles past the end of
an output, a workspace slice or a slab lands in memory the test owns and is reported, with the buffer it sits next to.  Every view
starts at a multiple of ALIGN bytes (what torch's allocator gives a tensor of its own), so alignment is not what is tested.

    out(*shape)     an output, pre-filled with PATTERN: check(written=[...]) then finds every element a kernel did not store
    inp(tensor)     a copy of an input: what lies behind its last element is PATTERN, not a plausible number, so a read past the
                    end that leaks into a sum shows as NaN in an output
    check(written=[...], untouched=[...])    after ONE synchronize: every guard is PATTERN; every element of every `written`
                    entry is not NaN; every element of every `untouched` entry still holds PATTERN -- an entry is a view, a slice
                    of one, or (tensor, mask) with a bool mask of the tensor's shape: what a kernel leaves alone by design is stated by the
                    test and pinned from both sides.  An AssertionError names the buffer and the first offending index.
    workspaces(KN)  context manager: kernels.tiled_ode_work and kernels._dopri5_tiled_work (torch.empty outside every arena)
                    return views of this arena, of the same size, PATTERN-filled and guarded; the arena keeps them until check()
    dopri5_records(KN)  context manager: the tensors of kernels.Dopri5Record (rec_y, rec_t, rec_h, fbuf, work; at construction and
                    in grow) are views of this arena, of the same shapes, PATTERN-filled and guarded, kept until check()
"""
import contextlib
from unittest import mock

import torch

F64 = torch.float64
GUARD = 512                                  # doubles of guard band before and behind every view (at least)
ALIGN = 256                                  # bytes: every view's address is a multiple of this
PATTERN = 0x7FF8BADC0FFEE0DD                 # a quiet NaN with a payload no arithmetic produces
CHUNK = 1 << 22                              # doubles of one backing buffer (a larger request gets a buffer of its own)


class _Chunk:
    def __init__(self, size, device):
        self.raw = torch.full((size,), PATTERN, dtype=torch.int64, device=device)
        self.f64 = self.raw.view(F64)
        self.guard = torch.ones(size, dtype=torch.bool, device=device)     # True: owned by no view
        self.cursor = 0                                                     # first element no view and no guard band has taken
        self.views = []                                                     # (start, size, name)

    def place(self, n):
        """offset of a view of n doubles: GUARD doubles behind the last one, rounded up to ALIGN bytes; None if it does not fit"""
        start = self.cursor + GUARD
        start += (-(self.raw.data_ptr() + 8 * start) % ALIGN) // 8
        return start if start + n + GUARD <= self.raw.numel() else None


class Arena:
    def __init__(self, device, chunk=CHUNK):
        self.device = torch.device(device)
        self.chunk = int(chunk)
        self.chunks = []
        self._n = 0

    # ---- allocation ---------------------------------------------------------------------------------------------------------
    def _view(self, shape, name):
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        c = self.chunks[-1] if self.chunks else None
        start = c.place(n) if c is not None else None
        if start is None:
            c = _Chunk(max(self.chunk, n + 2 * GUARD + ALIGN // 8), self.device)
            self.chunks.append(c)
            start = c.place(n)
        self._n += 1
        name = '%s#%d' % (name or 'buffer', self._n)
        c.views.append((start, n, name))
        c.guard[start:start + n] = False
        c.cursor = start + n
        v = c.f64[start:start + n].view(shape)
        assert v.is_contiguous() and v.data_ptr() % ALIGN == 0
        return v

    def out(self, *shape, name=None):
        """an output view of `shape`, every element PATTERN"""
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        return self._view(shape, name or 'out')

    def inp(self, tensor, name=None):
        """a guarded copy of an input (float64, contiguous)"""
        v = self._view(tensor.shape, name or 'inp')
        v.copy_(tensor.detach().to(F64))
        return v

    # ---- the workspace patch ------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def workspaces(self, KN):
        """kernels.tiled_ode_work / kernels._dopri5_tiled_work hand out guarded, PATTERN-filled views of this arena (same size)"""
        tiled, dopri = KN.tiled_ode_work, KN._dopri5_tiled_work

        def tiled_ode_work(*a, **kw):
            return self.out(tiled(*a, **kw).numel(), name='tiled_ode_work')

        def dopri5_tiled_work(*a, **kw):
            return self.out(dopri(*a, **kw).numel(), name='dopri5_tiled_work')

        with mock.patch.object(KN, 'tiled_ode_work', tiled_ode_work), mock.patch.object(KN, '_dopri5_tiled_work', dopri5_tiled_work):
            yield self

    @contextlib.contextmanager
    def dopri5_records(self, KN):
        """kernels.Dopri5Record keeps its tensors in this arena: rec_y, rec_t, rec_h, fbuf and work are views of the shapes the class
        itself gives them (torch.empty outside every arena), PATTERN-filled and guarded, at construction and again in grow(), which
        carries the first n_acc + 1 grid points over as the class does.  The arena keeps every generation until check(), so a store
        into a record that has been replaced still lands in memory the test owns.  Not covered: the per-launch controller rows and
        their page-locked mirror (torch.zeros / torch.empty inside kernels.dopri5_fwd) stay outside the arena."""
        arena, base = self, KN.Dopri5Record

        class GuardedRecord(base):
            FIELDS = ('rec_y', 'rec_t', 'rec_h', 'fbuf', 'work')

            def __init__(rec, *a, **kw):
                super().__init__(*a, **kw)
                for k in rec.FIELDS:
                    setattr(rec, k, arena.out(getattr(rec, k).shape, name='dopri5.' + k))

            def grow(rec, cap, n_acc):
                super().grow(cap, n_acc)                    # (new tensors outside the arena, the kept grid points copied in)
                for k, keep in (('rec_y', n_acc + 1), ('rec_t', n_acc + 1), ('rec_h', n_acc)):
                    new = getattr(rec, k)
                    v = arena.out(new.shape, name='dopri5.%s(cap %d)' % (k, cap))
                    v[:keep].copy_(new[:keep])
                    setattr(rec, k, v)

        with mock.patch.object(KN, 'Dopri5Record', GuardedRecord):
            yield self

    # ---- the checks ---------------------------------------------------------------------------------------------------------
    def _where(self, tensor):
        """(chunk, first element, name) of the view that holds `tensor`'s first element"""
        p = tensor.data_ptr()
        for c in self.chunks:
            base = c.raw.data_ptr()
            if base <= p < base + 8 * c.raw.numel():
                e = (p - base) // 8
                for start, n, name in c.views:
                    if start <= e < start + n:
                        return c, e, name
        raise AssertionError('a tensor given to Arena.check is not a view of this arena')

    @staticmethod
    def _first(bad):
        """index tuple of the first True of a bool tensor"""
        flat = int(torch.nonzero(bad.reshape(-1))[0])
        idx = []
        for s in reversed(bad.shape):
            idx.append(flat % s)
            flat //= s
        return tuple(reversed(idx))

    def check(self, written=(), untouched=()):
        if self.device.type == 'cuda':
            torch.cuda.synchronize()
        for ci, c in enumerate(self.chunks):
            bad = (c.raw != PATTERN) & c.guard
            if bool(bad.any()):
                e = int(torch.nonzero(bad)[0])
                before = [v for v in c.views if v[0] > e]
                behind = [v for v in c.views if v[0] + v[1] <= e]
                msgs = []
                if behind:
                    s, n, name = behind[-1]
                    msgs.append('%d doubles behind the end of %s' % (e - (s + n) + 1, name))
                if before:
                    s, n, name = before[0]
                    msgs.append('%d doubles before the start of %s' % (s - e, name))
                raise AssertionError('guard band overwritten (buffer %d, element %d: %s); %d guard elements changed in all'
                                     % (ci, e, ', '.join(msgs) or 'no view', int(bad.sum())))
        for entry in written:
            t, mask = entry if isinstance(entry, (tuple, list)) else (entry, None)
            _, _, name = self._where(t)
            bad = torch.isnan(t)
            if mask is not None:
                bad = bad & mask.to(bad.device)
            if bool(bad.any()):
                raise AssertionError('%s: element %s was not written (NaN); %d of %d elements are NaN'
                                     % (name, self._first(bad), int(bad.sum()), t.numel()))
        for entry in untouched:
            t, mask = entry if isinstance(entry, (tuple, list)) else (entry, None)
            _, _, name = self._where(t)
            bad = t.contiguous().view(torch.int64) != PATTERN
            if mask is not None:
                bad = bad & mask.to(bad.device)
            if bool(bad.any()):
                raise AssertionError('%s: element %s of a region the kernels leave untouched was overwritten; %d elements changed'
                                     % (name, self._first(bad), int(bad.sum())))
