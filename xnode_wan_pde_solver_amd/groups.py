"""Loading a sample into the engine: Group, Structure and GroupLoading, the base class of engine.Engine that holds its four
loaders.  The small rules they share are module-level functions: at_T0, start_values, batched_start_values, pair_terms, group_scalars.

Data layout in HBM (per group of N equal-length paths, L sample times, d dimensions):
  xT, xvT, xbT  float64 [d, N]   transposed coordinates of the u-, v- and boundary samples (the [N, L, d+1] path tensor
                                 of the reference is never materialised on the device: on vertical paths it is x (x) t)
  t             float64 [L]      shared time grid
  u, v, vt, f, ubar, vbar ...    float64 [L, N]   time-major point arrays (coalesced for one-lane-per-path kernels)
  Y             float64 [L, H, N]  hidden-state checkpoints of the stepper (written by the forward, read by the sweeps)
  act, act_b    float64 [L-1, rows, N]   stage activations of every step (forward -> sweeps: no field re-evaluation)
  vact          float64 [(q+1) W, N L]   layer inputs of the test network (its forward -> its backward)
  slabs         float64 [n_slab, P]  per-wave partial parameter gradients, summed inside the Adam kernel
"""
import math

import torch

from . import kernels as KN
from ._lib import XnwanError
from .sampling import _PIN_POOL, Hypercube, _paths

F32, F64 = torch.float32, torch.float64


def _d64(x, dev):
    """x on `dev` as float64; the tensor itself when it already is (two no-op .to() calls cost ~8 us of host time, and a
    list-domain sample makes ~400 of them)"""
    if x.dtype == F64 and x.device == dev:
        return x
    return x.to(dev).to(F64)


def _to_LN(x, dev):
    """[N, L] (any float dtype, any device) -> contiguous float64 [L, N] on dev"""
    return _d64(x.detach(), dev).t().contiguous()


class Structure:
    """What the PDE coefficient callables look like, found by probing them once on a few random points."""

    def __init__(self, funcs, d, lo=-1.0, hi=1.0):
        g = torch.Generator().manual_seed(20221111)
        Xp = torch.rand(6, 3, d + 1, generator=g) * (hi - lo) + lo
        Xp[:, :, 0] = torch.rand(6, 3, generator=g)
        ident = True
        for i in range(d):
            for j in range(d):
                a = funcs['a'](Xp, i, j)
                if not bool(torch.all(a == (1.0 if i == j else 0.0))):
                    ident = False
                    break
            if not ident:
                break
        self.a_identity = ident
        self.b_zero = all(bool(torch.all(funcs['b'](Xp, i) == 0)) for i in range(d))
        u1 = torch.randn(6, 3, 1, generator=g, dtype=F64)
        u2 = torch.randn(6, 3, 1, generator=g, dtype=F64)
        c1, c2 = funcs['c'](Xp, u1), funcs['c'](Xp.flip(0), u2)
        k = (c1 / u1).reshape(-1)
        self.c_kappa = None
        if torch.is_tensor(c1) and c1.shape == u1.shape and bool(torch.all(k == k[0])) and bool(torch.all(c2 == k[0] * u2)):
            self.c_kappa = float(k[0])

    def describe(self):
        return 'a=%s b=%s c=%s' % ('identity' if self.a_identity else 'general', 'zero' if self.b_zero else 'general',
                                   ('%g*u' % self.c_kappa) if self.c_kappa is not None else 'general')


class Group:
    """Device-resident data of one group of equal-length paths + every buffer its sub-steps need.  Buffers are allocated
    once and refilled in place by Engine.load_group(..., into=G), so captured HIP graphs stay valid across resampling."""
    SAMPLE_FIELDS = ('t', 'tb', 'tpp', 'tpp0', 'xvT_pts', 'xT', 'xvT', 'xbT', 'start', 'ghT', 'h', 'href', 'f', 'w', 'wt', 'w0', 'gwx0T',
                     'start_b', 'g', 'X', 'A0', 'B0')

    def signature(self):
        return tuple((k, tuple(getattr(self, k).shape)) for k in self.SAMPLE_FIELDS if getattr(self, k, None) is not None)

    # The work buffers are regions of ONE allocation (`_arena`), described by `_lazy` = {name: (offset, shape)}; the tensor
    # view of a region is made when somebody reads the attribute.  The sub-step runner only needs addresses (ptr): the groups
    # of a list domain are rebuilt with every sample, 19 groups x 22 buffers, and a torch.empty or a view costs the host 4 us each.
    def __getattr__(self, name):          # (only reached when the attribute is not set)
        lazy = self.__dict__.get('_lazy')
        if lazy is not None and name in lazy:
            off, shape = lazy[name]
            t = self.__dict__['_arena'][off:off + math.prod(shape)].view(shape)
            self.__dict__[name] = t
            return t
        raise AttributeError(name)

    def ptr(self, name):
        """device address of a buffer (0: the group has none)"""
        t = self.__dict__.get(name)
        if t is not None:
            return t.data_ptr()
        lazy = self.__dict__.get('_lazy')
        if lazy is not None and name in lazy:
            return self.__dict__['_arena'].data_ptr() + 8 * lazy[name][0]
        return 0


def at_T0(T0, hint=None, shared_grid_t0=None, grid=None, first=None):
    """Does a group start at T0 (start values h) or on the moving boundary (g)?  Decided HERE only, by the first source given:
    the first time of the ONE grid the caller built the sample from, the loader's host-side hint, the time column of the WHOLE
    group's first path (a rank's share may be empty or enter later), the tensor's own first time -- the only one that reads the
    device back, untouched when another is given.  By the loaders' contract (load_group) they all name the same number."""
    v = shared_grid_t0 if shared_grid_t0 is not None else hint if hint is not None else grid[0] if grid is not None else first
    return float(v) == T0


def start_values(funcs, P0, at_t0, want_grad):
    """the start values of a group on its first points P0 [N, d+1] -- h, or g on them as single-slice paths; with `want_grad`
    (s, their x-gradient [N, d]: the h -> y0 path of nabla_x u, src/model.py:95; zeros where s does not depend on P0)"""
    s = funcs['h'](P0) if at_t0 else funcs['g'](P0.unsqueeze(1)).reshape(-1)
    if not want_grad:
        return s
    return s, (torch.autograd.grad(s.sum(), P0)[0][:, 1:] if s.requires_grad else torch.zeros_like(P0[:, 1:]))


def batched_start_values(func_h, func_g, groups_first_points, at0):
    """start_values for all groups of a list sample in two calls: (P0, n, val) = the groups' first points [sum n, d+1] (a leaf
    that requires grad where a tape is recorded), their sizes, and the start values in group order.
    (h is evaluated ONLY on the start points of the groups that start at T0 and g ONLY on those that start on the
     boundary -- the combinations the per-group path evaluates: a callable that is not finite, or has no finite
     gradient, where it is never asked must not leak a NaN into the other groups through a masked merge)"""
    P0 = torch.cat(groups_first_points, 0)
    if torch.is_grad_enabled():
        P0 = P0.clone().requires_grad_(True)
    n = [x.shape[0] for x in groups_first_points]
    # (the groups are contiguous row ranges of P0: the rows of the groups that start at T0 / on the boundary are taken and
    #  put back as slices -- an index tensor would have to be uploaded or found on the device, both of which wait for
    #  everything queued on the stream, i.e. for the previous iteration's sub-steps when this runs beside them)
    rows = P0.split(n)
    rows_h, rows_g = ([r for r, a in zip(rows, at0) if a == want] for want in (True, False))
    some = lambda rows: sum(r.shape[0] for r in rows) > 0          # noqa: E731  (a rank's shares may hold none of them)
    hval = func_h(torch.cat(rows_h, 0)).reshape(-1) if some(rows_h) else None
    gval = func_g(torch.cat(rows_g, 0).unsqueeze(1)).reshape(-1) if some(rows_g) else None
    ref = hval if hval is not None else gval if gval is not None else P0
    none = ref.new_zeros(0)
    it_h = iter(hval.split([r.shape[0] for r in rows_h])) if hval is not None else iter([none] * len(rows_h))
    it_g = iter(gval.to(ref.dtype).split([r.shape[0] for r in rows_g])) if gval is not None else iter([none] * len(rows_g))
    return P0, n, torch.cat([next(it_h) if a else next(it_g) for a in at0], 0)


def pair_terms(h, f, g, nglob, nbglob, pair_i, pair_b, all_reduce=None):
    """Single-slice groups at T0: the reference's [N,N] broadcasts in factorised form.  The sums over m of the pair
    tables only involve the SAMPLE (h, f, g), so they are formed where it is loaded, once per sample:
      mean_nm (u_n - h_m)^2 = mean_n (u_n - mean h)^2 + var h          (src/loss.py:79; :84 likewise with g)
      sum_mn f_m phi_n      = N sum_n mean(f) phi_n                    (src/loss.py:70)
    -> (mean h, mean f, mean g, init_off = var h if pair_i, bdry_off = var g if pair_b) from ONE read-back of five sums.
    `all_reduce` (a sharded group): the means are over ALL nglob / nbglob paths of the group, not this rank's share."""
    zero = torch.zeros((), dtype=F64, device=h.device)
    gsum, gsq = (g.sum(), (g ** 2).sum()) if pair_b else (zero, zero)
    stats = torch.stack([h.sum(), (h ** 2).sum(), f.sum(), gsum, gsq]).contiguous()
    if all_reduce is not None:
        all_reduce(stats)
    sh, shh, sf, sg, sgg = stats.tolist()
    return (sh / nglob, sf / nglob, sg / nbglob, shh / nglob - (sh / nglob) ** 2 if pair_i else 0.0,
            sgg / nbglob - (sg / nbglob) ** 2 if pair_b else 0.0)


def group_scalars(G, old, domain, vol, N, L, Nb, Lb, n_glob, nb_glob, sharded, same_grid, amode, starts_T0, b_T0, pairwise, b_zero):
    """everything of a group that is not a tensor, set on the fresh Group G (`old`: the group it takes the place of, None: the
    first sample), for every loader; init_off / bdry_off are the loader's to set from pair_terms"""
    G.domain, G.N, G.L, G.Nb, G.Vol = domain, N, L, Nb, vol
    G.Nglob, G.Nbglob = float(n_glob if n_glob is not None else N), float(nb_glob if nb_glob is not None else max(Nb, 1))
    G.Lb, G.same_grid, G.amode = Lb, same_grid, amode
    # `sharded`: the sums of this group are partial sums (exchange steps in its sub-steps); `has_bdry`: the GROUP has boundary
    # paths, whether or not this rank holds any (which parameters Adam skips must not depend on the rank, _gen_back)
    G.sharded, G.has_bdry = sharded, (nb_glob if sharded else Nb) > 0
    G.pair_i = pairwise and L == 1 and starts_T0
    G.pair_b = pairwise and G.has_bdry and Lb == 1 and b_T0
    if G.pair_i and not b_zero:
        raise XnwanError('func_b != 0 on a single-slice group at T0: the reference sums that term with np.sum over a list of '
                         'tensors (src/loss.py:69), whose result on its [N,N] broadcast depends on the numpy version -- not '
                         'reproducible; set XW_ELEMENTWISE_SINGLE_SLICE=1 for the elementwise form')
    G.init_off, G.bdry_off, G.s3_scale, G.graphs = 0.0, 0.0, G.Nglob if G.pair_i else 1.0, {}
    # (a group of a list domain changes shape with every sample and is built anew each time: the count of samples it has seen
    #  is carried over, or the periodic structure guard -- two read-backs -- would run on EVERY sample)
    G.sample_version = old.sample_version + 1 if old is not None else 0


class GroupLoading:
    """The per-sample half of engine.Engine (parameter-independent, once per outer iteration): the user's callables tabulated
    and the groups of a sample loaded.  A base class: callers reach the loaders, packed_load, verify_every and _tab_cat on the
    engine.  It expects of the class it is mixed into (all set in Engine.__init__) the attributes dev, d, setup, funcs, world,
    structure, options (poison), verify_structure, verify_every, pairwise_single_slice, refill_variants, xproj_min_d,
    xproj_table_min_d and, for the work buffers, H, K, m, W, q, Pu, Pv, method, adjoint, keep_activations, testnet_tiled; and
    the methods _run (a captured or eager segment on a group), _side, _mark, _join (side streams), _form_xproj, _xproj_held and
    _v_key (the new sample's x-projection table).  It keeps _probe_u, _batch_tab, _batch_tab_checked and _tab_cat on it."""

    # ------------------------------------------------------------------------------------------------------------
    # coefficient tables (src/training.py:32-41).  Only time index 0 can contribute (Q3), so that slice is all that is
    # tabulated: [d,d,N] instead of the reference's [d,d,N,L].
    # ------------------------------------------------------------------------------------------------------------
    def _tabulate_a(self, X1):
        """a_ij(t_0, x_n) on the sample X1 [N,1,d+1], returned as (table, amode) -- the form is stated explicitly
        (xw_weak_contract_general's amode), never guessed from the shape: [d,d] and [d,N] coincide when N == d.  ONE batched call of the user's callable with index tensors
        i[d,1,1,1], j[1,d,1,1] when it is written with tensor operations (checked against scalar calls on three index
        pairs); otherwise the reference's d^2 scalar calls.  The table is then stored in the cheapest EXACT form: one
        [d,d] matrix if it does not vary over the sample, its diagonal [d,N] if every off-diagonal entry is exactly zero."""
        d, dev, fa = self.d, self.dev, self.funcs['a']
        N = X1.shape[0]
        A = None
        try:
            ii = torch.arange(d, device=X1.device).view(d, 1, 1, 1)
            jj = torch.arange(d, device=X1.device).view(1, d, 1, 1)
            out = fa(X1.unsqueeze(0).unsqueeze(0), ii, jj)
            if torch.is_tensor(out) and tuple(out.shape) == (d, d, N, 1):
                A = out[..., 0].to(dev).to(F32).to(F64)       # (the reference's table is float32: src/training.py:32)
                g = torch.Generator().manual_seed(d * 7919 + N)
                for _ in range(3):
                    i, j = (int(k) for k in torch.randint(0, d, (2,), generator=g))
                    if not torch.equal(A[i, j], fa(X1, i, j).to(dev).to(F32).to(F64)[:, 0]):
                        A = None
                        break
        except Exception:               # the callable branches on (i, j) in Python, indexes with them, ...: scalar calls
            A = None
        if A is None:
            A = torch.stack([torch.stack([fa(X1, i, j).to(dev).to(F32).to(F64)[:, 0] for j in range(d)], 0) for i in range(d)], 0)
        off = A.clone()
        off.diagonal(dim1=0, dim2=1).zero_()
        if bool(torch.all(A == A[:, :, :1])):
            return A[:, :, 0].contiguous(), 1                          # [d, d]   one matrix for all points
        if bool(torch.all(off == 0)):
            return A.diagonal(dim1=0, dim2=1).t().contiguous(), 2      # [d, N]   diagonal
        return A.contiguous(), 3                                       # [d, d, N] full table

    def _tabulate_b(self, X1):
        d, dev, fb = self.d, self.dev, self.funcs['b']
        N = X1.shape[0]
        try:
            out = fb(X1.unsqueeze(0), torch.arange(d, device=X1.device).view(d, 1, 1))
            if torch.is_tensor(out) and tuple(out.shape) == (d, N, 1):
                B = out[..., 0].to(dev).to(F32).to(F64)       # (float32 table: src/training.py:37)
                if all(torch.equal(B[i], fb(X1, i).to(dev).to(F32).to(F64)[:, 0]) for i in (0, d // 2, d - 1)):
                    return B.contiguous()
        except Exception:
            pass
        return torch.stack([fb(X1, i).to(dev).to(F32).to(F64)[:, 0] for i in range(d)], 0).contiguous()

    def _check_structure(self, X, version):
        """The fused fast paths (a = identity, b = 0, c = kappa u) were chosen from a probe on random points
        (Structure).  Guard them on the ACTUAL sample, every time one is loaded: the whole diagonal of a, one rotating
        off-diagonal per row (all pairs are visited over d samples), every b_i, and c against kappa u -- a coefficient
        that only deviates in part of the domain raises here instead of silently training the wrong PDE."""
        st, d = self.structure, self.d
        X1 = X[:, :1, :]
        bad = []                                   # (device-side flags, ONE host sync for the whole check)
        if st.a_identity:
            for i in range(d):
                j = (i + 1 + version % max(d - 1, 1)) % d
                bad.append(('func_a[%d,%d] == 1' % (i, i), torch.any(self.funcs['a'](X1, i, i) != 1)))
                if d > 1:
                    bad.append(('func_a[%d,%d] == 0' % (i, j), torch.any(self.funcs['a'](X1, i, j) != 0)))
        if st.b_zero:
            for i in range(d):
                bad.append(('func_b[%d] == 0' % i, torch.any(self.funcs['b'](X1, i) != 0)))
        if st.c_kappa is not None:
            key = (tuple(X.shape[:2]), str(X.device))
            if getattr(self, '_probe_u', (None, None))[0] != key:
                g = torch.Generator().manual_seed(1)
                self._probe_u = (key, torch.randn(X.shape[0], X.shape[1], 1, generator=g, dtype=F64).to(X.device))
            up = self._probe_u[1]
            bad.append(('func_c(X, u) == %g u' % st.c_kappa, torch.any(self.funcs['c'](X, up) != st.c_kappa * up)))
        # (results on the host cost nothing to read; results on the device are read back together: ONE sync)
        dev_flags = [b for _, b in bad if b.is_cuda]
        hit = any(bool(b) for _, b in bad if not b.is_cuda) or (bool(torch.stack(dev_flags).any()) if dev_flags else False)
        if hit:
            which = [name for name, b in bad if bool(b)]
            raise XnwanError('the PDE coefficients do not have the structure the probe at construction saw (%s): violated on this '
                             'sample: %s.  Build the solver with an explicit engine.Structure.' % (st.describe(), ', '.join(which[:4])))

    # ------------------------------------------------------------------------------------------------------------
    # per-sample preparation (once per outer iteration; everything here is parameter-independent)
    # ------------------------------------------------------------------------------------------------------------
    def tabulate_sample(self, triples, domain, hints=None, grids=None):
        """List domains (src/dataset.py:48-229: 11-20 groups per sample): evaluate the user's callables h, f, g and the
        domain's weight w (with their input gradients) ONCE on the points of ALL groups instead of group by group, and
        hand every group its slices (load_group(tab=...)).  The callables are PDE data -- functions of the point (t, x) --
        so evaluating them on a concatenation is the same arithmetic per point; that is CHECKED on the first group of the
        first sample (bitwise against the per-group call) and batching is switched off with a warning if it does not hold.
        Per outer iteration this removes ~140 of ~150 callable evaluations, each a dozen tiny kernel launches."""
        if getattr(self, '_batch_tab', True) is False or len(triples) < 2:
            return [None] * len(triples)
        if sum(t_[0].shape[0] for t_ in triples) == 0 or sum(t_[2].shape[0] for t_ in triples) == 0:
            return [None] * len(triples)      # (a rank whose shares of this sample hold no interior / no boundary path at all: group by group)
        d, T0 = self.d, self.setup['T0']
        Xs = [t_[0].detach() for t_ in triples]
        XVs = [t_[1].detach() for t_ in triples]
        BXs = [t_[2].detach() for t_ in triples]
        if hints is not None and all(h is not None for h in hints):      # (the loader read them off its host copies: no read-back)
            at0, bat0 = [at_T0(T0, hint=h['t0']) for h in hints], [at_T0(T0, hint=h['tb0']) for h in hints]
        else:
            # ONE host sync for all start times; a share of a sharded group reads the WHOLE group's first paths (`grids`: it may be
            # empty, or start at another path's entry time)
            gr = grids if grids is not None else [None] * len(Xs)
            if any(g_ is None and (x.shape[0] == 0 or b.shape[0] == 0) for g_, x, b in zip(gr, Xs, BXs)):
                raise XnwanError('tabulate_sample: an empty share needs the first times of the whole group (hints or grids)')
            first_t = torch.stack([(g_[0][0] if g_ is not None else x[0, 0, 0]).to(Xs[0].device) for g_, x in zip(gr, Xs)] +
                                  [(g_[1][0] if g_ is not None else b[0, 0, 0]).to(Xs[0].device) for g_, b in zip(gr, BXs)]).tolist()
            # (read back together, so the whole group's grid stands before the tensor's own first time HERE, as in at_T0)
            at0, bat0 = [at_T0(T0, first=v) for v in first_t[:len(Xs)]], [at_T0(T0, first=v) for v in first_t[len(Xs):]]
        pts = lambda ts: torch.cat([t_.reshape(-1, 1, d + 1) for t_ in ts], 0)                      # noqa: E731  [P, 1, d+1]
        cuts = lambda ts: [t_.shape[0] * t_.shape[1] for t_ in ts]                                  # noqa: E731
        f_cat = self.funcs['f'](pts(Xs)).detach().reshape(-1)
        g_cat = self.funcs['g'](pts(BXs)).detach().reshape(-1)
        f_all, g_all = f_cat.split(cuts(Xs)), g_cat.split(cuts(BXs))
        XVp = pts(XVs).clone().requires_grad_(True)
        w_all = domain.func_w(XVp)
        gw_all = torch.autograd.grad(w_all.sum(), XVp)[0] if w_all.requires_grad else torch.zeros_like(XVp)
        w_cat, gw_cat = w_all.detach().reshape(-1), gw_all.reshape(-1, d + 1)
        w_all, gw_all = w_cat.split(cuts(XVs)), gw_cat.split(cuts(XVs))
        # start values with their x-gradient: h for groups that start at T0, g for groups that start on the boundary
        X0, n0, start = batched_start_values(self.funcs['h'], self.funcs['g'], [x[:, 0, :] for x in Xs], at0)
        gh = torch.autograd.grad(start.sum(), X0)[0][:, 1:] if start.requires_grad else torch.zeros(X0.shape[0], d, device=X0.device, dtype=X0.dtype)
        # h on every interior start point (the s1 term and the initial penalty read it on all groups, src/loss.py:64,79;
        # for the groups that start at T0 it IS the start value)
        hv = start if all(at0) else self.funcs['h'](X0.detach()).reshape(-1)
        _, nb0, sb = batched_start_values(self.funcs['h'], self.funcs['g'], [b[:, 0, :] for b in BXs], bat0)
        sb = sb.detach()
        tabs = []
        # (the unsplit tables, for load_groups_packed: one gather launch takes every group's fields out of them)
        self._tab_cat = dict(f=f_cat, g=g_cat, w=w_cat, gw=gw_cat, start=start.detach(), gh=gh, h=hv.detach(), start_b=sb, at0=at0, bat0=bat0)
        start_k, gh_k, hv_k, sb_k = start.detach().split(n0), gh.split(n0), hv.detach().split(n0), sb.split(nb0)   # (once: a split is 20 new tensors)
        for k, (x, xv, bx) in enumerate(zip(Xs, XVs, BXs)):
            N, L = x.shape[0], x.shape[1]
            tabs.append(dict(starts_T0=at0[k], start=start_k[k], gh=gh_k[k], h=hv_k[k],
                             f=f_all[k].view(N, L), w=w_all[k].view(N, L), gw=gw_all[k].view(N, L, d + 1),
                             b_T0=bat0[k], start_b=sb_k[k], g=g_all[k].view(bx.shape[0], bx.shape[1])))
        if not getattr(self, '_batch_tab_checked', False):
            self._batch_tab_checked = True
            # bitwise against the per-group calls: f, h, w on the first group, and g, the start values with their gradient and the
            # boundary start values on the LAST triple (a late group: boundary-type starts on the hourglass)
            # (the first and the last group of which this rank holds interior AND boundary paths: an empty share has nothing to compare)
            full = [k for k in range(len(Xs)) if Xs[k].shape[0] > 0 and BXs[k].shape[0] > 0] or [0]
            k0, kl = full[0], full[-1]
            x, t0 = Xs[k0], tabs[k0]
            xl, bl, tl = Xs[kl], BXs[kl], tabs[kl]
            eq = lambda a, b: torch.equal(a.detach().reshape(-1), b.detach().reshape(-1))      # noqa: E731
            xl0 = xl[:, 0, :].clone().requires_grad_(True)
            s_l, g_l = start_values(self.funcs, xl0, at0[kl], True)
            sb_l = start_values(self.funcs, bl[:, 0, :], bat0[kl], False)
            if not (eq(self.funcs['f'](x), t0['f']) and eq(self.funcs['h'](x[:, 0, :]), t0['h']) and eq(domain.func_w(XVs[k0]), t0['w'])
                    and eq(self.funcs['g'](bl), tl['g']) and eq(s_l, tl['start']) and eq(g_l, tl['gh']) and eq(sb_l, tl['start_b'])):
                import warnings
                warnings.warn('the PDE callables give different values on a concatenation of groups than group by group (not pointwise?): '
                              'tabulating group by group', RuntimeWarning)
                self._batch_tab = False
                return [None] * len(triples)
        return tabs

    def load_group(self, X, XV, BX, domain, n_glob=None, nb_glob=None, into=None, shared_grid_t0=None, tab=None, verify=True,
                   hints=None, grids=None):
        """Prepare one group.  The user's callables (h, f, g, func_w, a, b) are evaluated on the device the given
        tensors live on and only their results are uploaded: pass the loader's host tensors to tabulate exactly like
        the reference's CPU path, or device tensors to tabulate on the GPU (float32 transcendental functions then
        differ from the host's in the last bit).  `into`: a Group of the same shapes to refill in place.
        `shared_grid_t0`: the caller built X, XV and BX from ONE time grid whose first time is this value (compact cube
        samples): the checks that would otherwise read the device tensors back (four host syncs) are skipped.
        `hints` (list domains, sampling.Comb_loader.pack): the same facts per group, read off the loader's HOST copies --
        `shared_times` (all paths of the group share one time column), `same_grid` (the boundary group sits on the
        interior group's grid).
        `n_glob`, `nb_glob` (several ranks): X, XV, BX are this rank's SHARE of a group of that many interior / boundary paths --
        the sub-steps of the group then run the exchange steps of dist.py; None: the whole group is here (one process, or a
        group every rank computes in full, dist.World.replicated).  A share may be empty ([0, L, d+1]: a group with fewer paths
        than ranks); `grids` = (time column of the WHOLE group's first interior path, of its first boundary path): the reference
        integrates every path of a group on its first path's grid (src/model.py:92: inputs[0, :, 0]), which an empty share does
        not hold and a later share holds a different one of where the paths of a group enter at their own times."""
        dev, d, T0 = self.dev, self.d, self.setup['T0']
        sharded = n_glob is not None and self.world is not None
        t0_hint, tb0_hint = (hints['t0'], hints.get('tb0')) if hints is not None else (None, None)      # (no boundary groups: no 'tb0')
        grid_i, grid_b = grids if grids is not None else (None, None)
        X, XV = X.detach(), XV.detach()
        BX = BX.detach() if BX is not None else None
        N, L = X.shape[0], X.shape[1]
        Nb = BX.shape[0] if BX is not None else 0
        if XV.shape[1] != L or XV.shape[0] != N:
            raise XnwanError('u- and v-samples of a group must have the same shape')
        if (N == 0 or (BX is not None and Nb == 0)) and not (sharded and grids is not None):
            raise XnwanError("a group without interior or boundary paths only exists as a rank's share of a sharded group (n_glob, grids)")
        S = {}
        S['t'] = _d64(grids[0] if grids is not None else X[0, :, 0], dev).contiguous()
        S['xT'] = _d64(X[:, 0, 1:], dev).t().contiguous()
        S['xvT'] = _d64(XV[:, 0, 1:], dev).t().contiguous()
        # the test network is pointwise on XV: when the paths of a group do not share one time column (late-entry groups
        # of the hourglass: every path has its own entry time at l = 0) it runs in point mode on all L*N points
        S['tpp'] = S['tpp0'] = S['xvT_pts'] = None
        # (a share of a sharded group is compared with the WHOLE group's first path, whose grid G.t is: `grids`)
        col0 = XV[:1, :, 0] if grids is None else grids[0].to(XV.device).view(1, -1)
        if shared_grid_t0 is None and not (hints['shared_times'] if hints is not None else bool(torch.all(XV[:, :, 0] == col0))):
            S['tpp'] = _d64(XV[:, :, 0], dev).t().contiguous().reshape(-1)              # time-major: p = l*N + n
            S['tpp0'] = _d64(XV[:, 0, 0], dev).contiguous()
            S['xvT_pts'] = S['xvT'].unsqueeze(1).expand(d, L, N).reshape(d, L * N).contiguous()
        # start values and their x-gradient (the h -> y0 path of nabla_x u, src/model.py:95)
        # (an empty share holds no first time of its own: the earlier sources of at_T0 say it)
        starts_T0 = bool(tab['starts_T0']) if tab is not None else at_T0(T0, t0_hint, shared_grid_t0, grid_i, X[0, 0, 0] if N else None)
        if tab is not None:                   # (tabulate_sample: evaluated once for all groups of the sample)
            S['start'] = _d64(tab['start'], dev).reshape(-1).contiguous()
            S['ghT'] = _d64(tab['gh'], dev).t().contiguous()
            S['h'] = _d64(tab['h'], dev).reshape(-1).contiguous()
            S['f'] = _to_LN(tab['f'], dev)
            w, gw = tab['w'], tab['gw']
        elif N == 0:
            # an empty share: the user's callables are not asked about no points (max(), indexing ... of an empty tensor)
            z = lambda *shape: torch.zeros(*shape, dtype=F64, device=dev)  # noqa: E731
            S['start'], S['ghT'], S['h'], S['f'] = z(0), z(d, 0), z(0), z(L, 0)
            Lw = 1 if getattr(domain, 'time_independent', False) else L
            w, gw = z(0, Lw), z(0, Lw, d + 1)
        else:
            X0 = X[:, 0, :].clone().requires_grad_(True)
            s, gs = start_values(self.funcs, X0, starts_T0, True)
            S['start'] = _d64(s.detach(), dev).reshape(-1).contiguous()
            S['ghT'] = gs.to(dev).to(F64).t().contiguous()
            # (a group that starts at T0: h(X[:, 0, :]) is the start value itself)
            S['h'] = S['start'] if starts_T0 else self.funcs['h'](X[:, 0, :]).detach().to(dev).to(F64).reshape(-1).contiguous()
            S['f'] = _to_LN(self.funcs['f'](X), dev)
            # distance weight on the v-sample and its gradient (nabla phi = w nabla v + v nabla w, src/loss.py:51-63): in
            # closed form where the domain offers it (identical to autograd's, ties included), on the first time slice only
            # where w does not depend on time
            XVw = XV[:, :1] if getattr(domain, 'time_independent', False) else XV
            if hasattr(domain, 'func_w_grad'):
                w, gw = domain.func_w_grad(XVw)
            else:
                XVl = XVw.clone().requires_grad_(True)
                w = domain.func_w(XVl)
                gw = torch.autograd.grad(w.sum(), XVl)[0] if w.requires_grad else torch.zeros_like(XVl)
        if getattr(domain, 'time_independent', False):
            S['w'] = _d64(w[:, 0].detach(), dev).contiguous()
            S['wt'] = None
        else:
            S['w'] = _to_LN(w, dev)
            S['wt'] = _to_LN(gw[:, :, 0], dev)
        S['w0'] = _d64(w[:, 0].detach(), dev).contiguous()
        S['gwx0T'] = _d64(gw[:, 0, 1:], dev).t().contiguous()
        S['xbT'] = S['start_b'] = S['g'] = S['tb'] = None
        Lb, same_grid, b_T0 = 0, True, False
        if BX is not None:
            Lb = BX.shape[1]
            S['tb'] = _d64(grids[1] if grids is not None else BX[0, :, 0], dev).contiguous()
            same_grid = Lb == L and (shared_grid_t0 is not None or (hints['same_grid'] if hints is not None else bool(torch.equal(S['tb'], S['t']))))
            S['xbT'] = _d64(BX[:, 0, 1:], dev).t().contiguous()
            b_T0 = bool(tab['b_T0']) if tab is not None else at_T0(T0, tb0_hint, shared_grid_t0, grid_b, BX[0, 0, 0] if Nb else None)
            if tab is not None:
                S['start_b'] = _d64(tab['start_b'], dev).reshape(-1).contiguous()
                S['g'] = _to_LN(tab['g'], dev)
            elif Nb == 0:
                S['start_b'], S['g'] = torch.zeros(0, dtype=F64, device=dev), torch.zeros(Lb, 0, dtype=F64, device=dev)
            else:
                sb = start_values(self.funcs, BX[:, 0, :], b_T0, False)
                S['start_b'] = _d64(sb.detach(), dev).reshape(-1).contiguous()
                S['g'] = _to_LN(self.funcs['g'](BX), dev)
        st = self.structure
        S['X'] = X.to(dev) if st.c_kappa is None else None      # only read by a general reaction callable c(u, t, x)
        S['A0'] = S['B0'] = None
        amode = 0
        if not st.a_identity and N > 0:
            S['A0'], amode = self._tabulate_a(X[:, :1, :])     # [d,d,N] / [d,N] (diagonal) / [d,d] (constant) at time index 0
        if not st.b_zero and N > 0:
            S['B0'] = self._tabulate_b(X[:, :1, :])            # [d, N]
        if verify and N > 0:
            self._guard(into, lambda: X)
        fresh = Group()
        group_scalars(fresh, into, domain, float(domain.V()), N, L, Nb, Lb, n_glob, nb_glob, sharded, same_grid, amode, starts_T0, b_T0,
                      self.pairwise_single_slice, st.b_zero)
        S['href'] = None
        if fresh.pair_i or fresh.pair_b:
            mean_h, mean_f, mean_g, fresh.init_off, fresh.bdry_off = pair_terms(
                S['h'], S['f'], S['g'], fresh.Nglob, fresh.Nbglob, fresh.pair_i, fresh.pair_b, self.world.all_reduce if sharded else None)
            if fresh.pair_i:
                S['href'] = torch.full((N,), mean_h, dtype=F64, device=dev)
                S['f'] = torch.full_like(S['f'], mean_f)
            if fresh.pair_b:
                S['g'] = torch.full_like(S['g'], mean_g)
        if into is not None:
            G = into
            same = all(getattr(G, k) == getattr(fresh, k) for k in ('N', 'L', 'Nb', 'Lb', 'same_grid', 'Vol', 'Nglob', 'Nbglob', 'pair_i',
                                                                     'pair_b', 'amode', 'sharded')) and all(
                (getattr(G, k) is None) == (S[k] is None) and (S[k] is None or getattr(G, k).shape == S[k].shape)
                for k in Group.SAMPLE_FIELDS)
            if same:
                for k in Group.SAMPLE_FIELDS:
                    if S[k] is not None:
                        getattr(G, k).copy_(S[k])
                G.__dict__.update(fresh.__dict__, graphs=G.graphs)      # (the scalars of the new sample; the captured graphs stay valid)
                self._form_xproj(G)
                return G
        G = fresh
        for k in Group.SAMPLE_FIELDS:
            setattr(G, k, S[k])
        # work buffers
        # XW_POISON=1 (debugging): work buffers start as NaN instead of whatever the allocator hands out, so that a kernel
        # reading a slot nobody wrote shows up as NaN in the results instead of as a stale, plausible number
        self._work_buffers(G, [])
        self._form_xproj(G)
        return G

    def _guard(self, old, sample):
        """_check_structure on sample() where it is due: on the first sample of a group (`old`: the group the new one takes the
        place of, None: none) and on every verify_every-th after it"""
        ver = old.sample_version if old is not None else 0
        if self.verify_structure and ver % self.verify_every == 0:
            self._check_structure(sample(), ver // self.verify_every)

    def load_groups_packed(self, shards, hints, domain, cache, big):
        """load_group for ALL groups of a list-domain sample at once (time-varying balls: 11-20 groups): every sample field of
        every group is a strided view of the uploaded sample or of a table tabulate_sample has just filled for the whole
        sample, so the fields are regions of each group's one allocation (Group._arena) and ONE gather launch
        (kernels.gather_fields, a ~350-row table uploaded once) fills them -- instead of ~45 tensor operations per group.
        Same values bit for bit (copies), same Group attributes.  Returns None when the sample is not of that kind (anything
        but float64 device tensors, general a / b / c, no batched tabulation): the caller goes group by group.
        `shards`: (X, XV, BX, n_glob, nb_glob, grids) per group as in load_group -- with several ranks this rank's shares (possibly
        empty) of the groups that are sharded, the whole of those that are replicated."""
        tc = getattr(self, '_tab_cat', None)
        st = self.structure
        if (tc is None or not (st.a_identity and st.b_zero and st.c_kappa is not None)
                or getattr(domain, 'time_independent', False) or any(h is None for h in hints)):
            return None
        srcs = [tc[k] for k in ('f', 'g', 'w', 'gw', 'start', 'gh', 'h', 'start_b')]
        if any(t.dtype != F64 or not t.is_cuda for t in srcs) or any(t.dtype != F64 or not t.is_cuda or t_[0] is not t_[1]
                                                                       for t_ in shards for t in t_[:3]):
            return None
        d, dev = self.d, self.dev
        f_cat, g_cat, w_cat, gw_cat, start, gh, hv, sb = srcs
        if f_cat.stride(0) != 1 or g_cat.stride(0) != 1 or w_cat.stride(0) != 1:
            return None
        g0, g1 = gw_cat.stride()
        h0, h1 = gh.stride()
        rows, groups, total = [], [], 0
        oN = oNL = oNb = oNbL = 0
        vol = float(domain.V())
        for k, ((X, XV, BX, n_glob, nb_glob, grids), hn) in enumerate(zip(shards, hints)):
            N, L, Nb, Lb = X.shape[0], X.shape[1], BX.shape[0], BX.shape[1]
            sharded = n_glob is not None and self.world is not None
            shared = bool(hn['shared_times'])
            same_grid = Lb == L and bool(hn['same_grid'])
            old = cache[k] if k < len(cache) else None
            G = Group()
            group_scalars(G, old, domain, vol, N, L, Nb, Lb, n_glob, nb_glob, sharded, same_grid, 0, bool(tc['at0'][k]), bool(tc['bat0'][k]),
                          self.pairwise_single_slice, st.b_zero)
            fields = [('t', (L,)), ('xT', (d, N))]
            if not shared:
                fields += [('tpp', (L * N,)), ('tpp0', (N,)), ('xvT_pts', (d, L * N))]
            fields += [('start', (N,)), ('ghT', (d, N)), ('h', (N,)), ('f', (L, N)), ('w', (L, N)), ('wt', (L, N)), ('w0', (N,)), ('gwx0T', (d, N)),
                       ('tb', (Lb,)), ('xbT', (d, Nb)), ('start_b', (Nb,)), ('g', (Lb, Nb))]
            self._work_buffers(G, fields, cached_table=False)
            G._lazy['xvT'] = G._lazy['xT']           # (the v sample of a list domain is the u sample)
            if shared:
                G.tpp = G.tpp0 = G.xvT_pts = None
            G.href = G.X = G.A0 = G.B0 = None
            base = G._arena.data_ptr()
            x0, x1, x2 = X.stride()
            b0, b1, b2 = BX.stride()
            xp, bp = X.data_ptr(), BX.data_ptr()
            # (the grids are those of the WHOLE group's first paths: load_group)
            t_src = (xp, x1) if grids is None else (grids[0].data_ptr(), grids[0].stride(0))
            tb_src = (bp, b1) if grids is None else (grids[1].data_ptr(), grids[1].stride(0))
            src = {'t': (t_src[0], 1, 1, L, 0, 0, t_src[1]), 'xT': (xp + 8 * x2, 1, d, N, 0, x2, x0),
                   'tpp': (xp, 1, L, N, 0, x1, x0), 'tpp0': (xp, 1, 1, N, 0, 0, x0), 'xvT_pts': (xp + 8 * x2, d, L, N, x2, 0, x0),
                   'start': (start.data_ptr() + 8 * oN * start.stride(0), 1, 1, N, 0, 0, start.stride(0)),
                   'ghT': (gh.data_ptr() + 8 * oN * h0, 1, d, N, 0, h1, h0),
                   'h': (hv.data_ptr() + 8 * oN * hv.stride(0), 1, 1, N, 0, 0, hv.stride(0)),
                   'f': (f_cat.data_ptr() + 8 * oNL, 1, L, N, 0, 1, L),
                   'w': (w_cat.data_ptr() + 8 * oNL, 1, L, N, 0, 1, L),
                   'wt': (gw_cat.data_ptr() + 8 * oNL * g0, 1, L, N, 0, g0, L * g0),
                   'w0': (w_cat.data_ptr() + 8 * oNL, 1, 1, N, 0, 0, L),
                   'gwx0T': (gw_cat.data_ptr() + 8 * (oNL * g0 + g1), 1, d, N, 0, g1, L * g0),
                   'tb': (tb_src[0], 1, 1, Lb, 0, 0, tb_src[1]), 'xbT': (bp + 8 * b2, 1, d, Nb, 0, b2, b0),
                   'start_b': (sb.data_ptr() + 8 * oNb * sb.stride(0), 1, 1, Nb, 0, 0, sb.stride(0)),
                   'g': (g_cat.data_ptr() + 8 * oNbL, 1, Lb, Nb, 0, 1, Lb)}
            for name, shape in fields:
                a, n0_, n1_, n2_, s0_, s1_, s2_ = src[name]
                if n0_ * n1_ * n2_ == 0:        # (an empty share: nothing to gather)
                    continue
                rows.append((a, base + 8 * G._lazy[name][0], n0_, n1_, n2_, s0_, s1_, s2_, total))
                total += n0_ * n1_ * n2_
            if k == big:
                self._guard(old, lambda: X)
            groups.append(G)
            oN, oNL, oNb, oNbL = oN + N, oNL + N * L, oNb + Nb, oNbL + Nb * Lb
        if len(rows) > KN.GATHER_ROWS:
            return None
        table = torch.zeros(KN.GATHER_ROWS, 9, dtype=torch.int64)
        table[:len(rows)] = torch.tensor(rows, dtype=torch.int64)
        pinned = _PIN_POOL.stage(table)
        tdev = pinned.to(dev, non_blocking=True)
        _PIN_POOL.uploaded(pinned, torch.cuda.current_stream(dev))
        KN.gather_fields(tdev, len(rows), total)
        for G in groups:
            self._form_xproj(G)
        # single-slice groups at T0: the reference's [N, N] broadcasts in factorised form (pair_terms); these read five sums back
        for G in groups:
            if G.pair_i or G.pair_b:
                mean_h, mean_f, mean_g, G.init_off, G.bdry_off = pair_terms(
                    G.h, G.f, G.g, G.Nglob, G.Nbglob, G.pair_i, G.pair_b, self.world.all_reduce if G.sharded else None)
                if G.pair_i:
                    G.href = torch.full((G.N,), mean_h, dtype=F64, device=dev)
                    G.f.fill_(mean_f)
                if G.pair_b:
                    G.g.fill_(mean_g)
        return groups

    def _work_buffers(self, G, fields, cached_table=True):
        """every buffer the sub-steps of G need, as regions of ONE allocation (Group._arena / _lazy), behind the regions `fields`
        = [(name, shape)] the caller fills itself (load_groups_packed: the sample fields)"""
        dev, d, N, L, Nb, Lb = self.dev, self.d, G.N, G.L, G.Nb, G.Lb
        poison = self.options.poison
        H = self.H
        # stage activations of every step, written by the forward, read back by the sweeps (183 MB at N = 4096, L = 32)
        ar = KN.ode_act_rows(self.method, H, self.K, self.m) if self.keep_activations and not self.adjoint else 0
        # layer inputs of the test network at every point, stored by its forward in the discriminator sub-step and read
        # back by its backward (524 MB at 131072 points)
        # (only the reference's width and depth have a recomputing reverse kernel: everything else always runs from the record)
        keep_v = self.keep_activations or self.testnet_tiled or not KN.disc_recompute(self.W, self.q)
        G.ns_u = KN.ode_bwd_slabs(N)
        G.ns_b = KN.ode_bwd_slabs(Nb) if Nb else 0
        nw = KN.reduce_work_size()
        plan = list(fields) + [('u', (L, N)), ('Y', (L, H, N)), ('v', (L, N)), ('vt', (L, N)), ('gxv', (d, N)), ('gtv', (N,)), ('gx', (d, N)), ('gs', (N,)),
                ('vbar', (L, N)), ('s3x', (N,)),
                ('slabA', (G.ns_u + G.ns_b, self.Pu)),         # sweep with cotangent A (interior) + the boundary sweep
                ('slabB', (G.ns_u, self.Pu)),                  # sweep with cotangent B = dI/du
                ('slab_v', (KN.disc_bwd_slabs(N, L), self.Pv)),
                ('work_i', (nw,)), ('work_b', (nw,))]          # scratch of the deterministic grid sums (interior / boundary run concurrently): zeroed below
        if ar:
            plan.append(('act', (max(L - 1, 1), ar, KN.ode_act_cols(N))))
            if Nb:
                plan.append(('act_b', (max(Lb - 1, 1), ar, KN.ode_act_cols(Nb))))
        if keep_v:
            plan.append(('vact', (KN.disc_act_rows(self.W, self.q), KN.disc_act_cols(L * N))))
        # (below xproj_min_d the table only pays without its head launch: path-mode groups, whose table is cached)
        point_mode = G.__dict__.get('tpp') is not None or any(n_ == 'tpp' for n_, _ in fields)
        if N and (d >= self.xproj_min_d or (cached_table and d >= self.xproj_table_min_d and not point_mode)):
            plan.append(('xproj', (KN.disc_xproj_rows(self.W), N)))   # Vin[:, 1..d] x + Vin.b per path (_launch_test_net_here)
        if Nb:
            plan += [('ub', (Lb, Nb)), ('Yb', (Lb, H, Nb))]
        lazy, off = {}, 0
        for name, shape in plan:
            lazy[name] = (off, shape)
            off += -(-math.prod(shape) // 64) * 64           # (regions start on 512-byte boundaries, like allocations of their own)
        G._arena = torch.full((off,), float('nan'), dtype=F64, device=dev) if poison else torch.empty(off, dtype=F64, device=dev)
        G._lazy = lazy
        w0 = lazy['work_i'][0]
        G._arena[w0:lazy['work_b'][0] + nw].zero_()
        G.c = G.cp = None
        if not ar:
            G.act = G.act_b = None
        elif not Nb:
            G.act_b = None
        if not keep_v:
            G.vact = None

    def refill_compact(self, G, comp, domain, n_glob=None, nb_glob=None):
        """load_group(..., into=G) for a COMPACT sample of a domain whose paths are vertical lines over one shared grid
        (times [L], x_u [N, d], x_v [N, d], x_b [N_b, d]; host tensors, page-locked ones upload asynchronously): the
        sample goes into four static device buffers and everything load_group does with it on the device -- the path
        tensors, the callables h (with its gradient), f, g, the domain's weight, the transposes and conversions into the
        group's sample fields, ~110 small kernels -- is captured ONCE per shape into a HIP graph and replayed: an outer
        iteration of train() at the headline size spent 1.0 of its 2.4 ms of host time issuing them one by one.  Same
        rule as the sub-step graphs (_run): a callable that cannot be captured (it syncs with the host) makes this
        segment eager, with a warning.  The guard on the probed coefficient structure stays outside the graph."""
        times = comp[0]
        st = G.__dict__.get('_refill_in')
        if st is None or any(a.shape != b.shape or a.dtype != b.dtype for a, b in zip(st, comp)):
            st = G._refill_in = [torch.empty(tuple(c.shape), dtype=c.dtype, device=self.dev) for c in comp]
            G.graphs = {k: v for k, v in G.graphs.items() if not k.startswith('refill')}
        for dst, src in zip(st, comp):
            dst.copy_(src, non_blocking=True)
        _PIN_POOL.uploaded_all(comp, torch.cuda.current_stream(self.dev))
        t0 = float(times[0])                                   # (host tensor: no device read-back)
        td, du, dv, db = st
        ver = G.sample_version
        self._guard(G, lambda: _paths(td, du))

        lean = (self.structure.a_identity and self.structure.b_zero and self.structure.c_kappa is not None
                and getattr(domain, 'time_independent', False) and hasattr(domain, 'func_w_grad') and G.Nb > 0 and G.same_grid
                and not (G.pair_i or G.pair_b) and G.tpp is None
                and (G.N, G.L, G.Nb, G.Lb) == (du.shape[0], td.shape[0], db.shape[0], td.shape[0])
                and float(domain.V()) == G.Vol and n_glob in (None, G.Nglob) and nb_glob in (None, G.Nbglob))

        def body(_G):
            if lean:
                self._refill_fields(G, td, du, dv, db, domain, t0)
                self._form_xproj(G)      # (the new sample's table, part of the refill graph: outside every sub-step)
                return
            out = self.load_group(_paths(td, du), _paths(td, dv), _paths(td, db), domain, n_glob, nb_glob, into=G, shared_grid_t0=t0,
                                  verify=False)
            if out is not G:
                raise XnwanError('refill_compact: the sample does not have the shapes of the group it refills')
        # (what the captured body bakes in besides the buffers: the grid's first time, the domain's class and extent, which of
        #  the two bodies it is and the global path counts)
        key = 'refill_%r_%s_%r_%r_%r_%d_%r_%r' % (t0, type(domain).__name__, float(domain.V()), getattr(domain, 'top', None),
                                                  getattr(domain, 'bot', None), int(lean), n_glob, nb_glob)
        if key not in G.graphs and sum(1 for k in G.graphs if k.startswith('refill')) >= self.refill_variants:
            # a domain whose first time or extent changes with every sample would capture a graph per outer iteration (graphs are
            # never destroyed, _KEPT_GRAPHS): beyond a few variants per group the refill runs eagerly
            if not G.__dict__.get('_refill_cap_warned'):
                import warnings
                G._refill_cap_warned = True
                warnings.warn('more than %d variants of the refill graph for one group (first time / extent / path counts change from '
                              'sample to sample): further variants run as eager launches' % self.refill_variants, RuntimeWarning, stacklevel=2)
            G.graphs[key] = False
        self._run(G, key, body, scratch=True)
        # (host-side bookkeeping of load_group: done at capture time only, so it is set here on every path)
        G.domain, G.sample_version = domain, ver + 1
        if self._xproj_held(G):
            G.xproj_key = self._v_key(G)
        return G

    def _refill_fields(self, G, td, du, dv, db, domain, t0):
        """What load_group(paths(td, du), paths(td, dv), paths(td, db), into=G, shared_grid_t0=t0) writes into the sample
        fields of a group of vertical paths over ONE grid, on a time-independent domain with the fused coefficient structure
        (a = identity, b = 0, c = kappa u) -- the same values bit for bit (the same callables on the same tensors; every
        conversion is an exact float32 -> float64 widening or a transpose), written straight into the fields: a widening, a
        transpose and the copy into the field are ONE strided copy here and three kernels there (~110 -> ~85 per sample).
        The four independent chains -- f on the interior paths | the start values h with their gradient | the domain's
        weight | the boundary paths -- run on the engine's side streams: captured (refill_compact), that makes them
        parallel branches of the graph, and the GPU has nothing else to do between two outer iterations."""
        fn = self.funcs
        at0 = at_T0(self.setup['T0'], shared_grid_t0=t0)
        e0 = self._mark()
        with self._side(1, e0):                       # start values and their x-gradient (the h -> y0 path of nabla_x u)
            X0 = _paths(td[:1], du)[:, 0, :].requires_grad_(True)
            s_, gs = start_values(fn, X0, at0, True)
            G.start.copy_(s_.detach().reshape(-1))
            G.ghT.copy_(gs.t())
            # (a group that starts at T0: h on its first points IS the start value)
            G.h.copy_(G.start if at0 else fn['h'](X0.detach()).reshape(-1))
            e1 = self._mark()
        with self._side(2, e0):                       # distance weight on the v-sample, first time slice (time-independent)
            stock = type(domain).func_w_grad is Hypercube.func_w_grad and type(domain).func_w is Hypercube.func_w
            if stock and dv.dtype == F32 and dv.is_contiguous():
                # the stock hypercube: its weight, the gradient and the transposed points in ONE launch (xw_cube_weight: same
                # float32 arithmetic, same tie rules as the tensor formulation below, which takes 29)
                KN.cube_weight(dv, domain.top, domain.bot, G.w, G.gwx0T, w0=G.w0, xT=G.xvT)
            else:
                w, gw = domain.func_w_grad(_paths(td[:1], dv))
                G.w.copy_(w[:, 0].detach())
                G.w0.copy_(w[:, 0].detach())
                G.gwx0T.copy_(gw[:, 0, 1:].t())
                G.xvT.copy_(dv.t())
            e2 = self._mark()
        with self._side(3, e0):                       # boundary paths
            BX = _paths(td, db)
            sb = start_values(fn, BX[:, 0, :], at0, False)
            G.start_b.copy_(sb.detach().reshape(-1))
            G.g.copy_(fn['g'](BX).detach().t())
            G.xbT.copy_(db.t())
            G.tb.copy_(td)
            e3 = self._mark()
        G.t.copy_(td)
        G.xT.copy_(du.t())
        G.f.copy_(fn['f'](_paths(td, du)).detach().t())
        self._join(e1, e2, e3)
