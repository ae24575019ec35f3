"""The test network's x-projection table kept per group (EngineOptions.xproj_cached): formed where the sample is loaded and right
behind the discriminator's Adam instead of at the head of every test-network launch.

The cached table holds the bits of a table formed at the head -- the same kernel on the same inputs -- so every comparison here is
bit for bit, against an engine that forms it at the head (`xproj_min_d=1, xproj_cached=False`: the path the suite already checks
against the oracle).  Shapes: d = 5, N = 33 (three 16-point tiles per time, the last ragged), N_b = 17, L = 3, shallow networks,
test network 50 wide and 64 wide (the two containers whose input layer can also run per point): the smallest at which a stale or
misplaced table shows.  The cached engines run `xproj_cached_min_d=1`: the switch itself stays at its default (on), the table is
forced at this small d like `xproj_min_d=1` forces it for the uncached ones."""
import numpy as np
import pytest
import torch

import configs.Ex4_1_funcs as P
from guarded import Arena

pytestmark = pytest.mark.gpu

SEQ = 'ggdgd'
CACHED = dict(xproj_cached_min_d=1)
AT_HEAD = dict(xproj_min_d=1, xproj_cached=False)


def _params(W, **kw):
    p = {'alpha': 1e4, 'u_layers': 2, 'u_hidden_dim': 20, 'u_hidden_hidden_dim': 10, 'v_layers': 3, 'v_hidden_dim': W,
         'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'midpoint',
         'dim': 5, 'N_t': 3, 'N_r': 33, 'N_b': 17, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 1, 'domain': 'Hypercube'}
    p.update(kw)
    return p


@pytest.fixture(scope='module')
def sample():
    """ONE sample (and a second one for the resampling case) shared by every engine of this module; never written to"""
    from src.dataset import Comb_loader
    from xnode_wan_pde_solver_amd import sampling
    torch.manual_seed(11)
    s = _params(50)
    domain = sampling.Hypercube(s['shape_param'], s['dim'], s['T0'], s['T'], s['N_t'])
    dev = torch.device('cuda')
    return domain, Comb_loader(s['N_r'], s['N_b'], domain, dev), Comb_loader(s['N_r'], s['N_b'], domain, dev)


def _engine(W, **opts):
    from src.training import NODE_WAN_solver
    from xnode_wan_pde_solver_amd.options import EngineOptions
    params = opts.pop('params', None) or _params(W)
    torch.manual_seed(3)
    np.random.seed(3)
    S = NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, torch.device('cuda'), './',
                        func_u_sol=P.func_u_sol, p=2, options=EngineOptions(**opts))
    return S


def _load(S, sample, which=1, into=None):
    domain, pts = sample[0], sample[which]
    return S.engine.load_group(pts.interioru, pts.interiorv, pts.boundary, domain, into=into)


def _state(eng):
    torch.cuda.synchronize()
    return [t.clone() for t in (eng.theta.data, eng.phi.data, eng.loss_u().reshape(1), eng.loss_v().reshape(1), eng.grad_u, eng.grad_v)]


NAMES = ('theta', 'phi', 'loss_u', 'loss_v', 'grad_u', 'grad_v')


def _run(eng, G, seq=SEQ, between=None):
    """the state after every sub-step of `seq`; between[i](): an event in front of sub-step i"""
    out = []
    for i, c in enumerate(seq):
        if between and i in between:
            between[i]()
        (eng.generator_step if c == 'g' else eng.discriminator_step)(G)
        out.append(_state(eng))
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (sa, sb) in enumerate(zip(a, b)):
        for n, x, y in zip(NAMES, sa, sb):
            assert torch.equal(x, y), '%s: %s differs after sub-step %d (max |diff| %.3e)' % (what, n, i, float((x - y).abs().max()))
        assert all(bool(torch.isfinite(x).all()) for x in sa)


@pytest.mark.parametrize('W', [50, 64])
def test_cached_table_against_a_table_formed_at_every_head(sample, W):
    """g, g, d, g, d: theta, phi, the losses and both gradients bit-identical after every sub-step.  The generator sub-step behind a
    discriminator one is what catches a table formed before Adam instead of behind it."""
    runs = []
    for opts in (CACHED, AT_HEAD):
        S = _engine(W, **opts)
        G = _load(S, sample)
        assert G.ptr('xproj') != 0 and G.tpp is None
        runs.append(_run(S.engine, G))
        if opts is CACHED:
            # captured: every graph of this group is one without the head node
            assert S.engine.xproj_cached and sorted(G.graphs) == ['disc_act_xc', 'gen_xc'], sorted(G.graphs)
            assert 'cached' in S.plan()['testnet_input_layer']
        else:
            assert not S.engine.xproj_cached and not any(k.endswith('_xc') for k in G.graphs)
            assert 'head of every' in S.plan()['testnet_input_layer']
    _same(runs[0], runs[1], 'cached against formed at the head, W = %d' % W)
    assert not torch.equal(runs[0][1][1], runs[0][2][1])          # (phi does move in the discriminator sub-step)


@pytest.mark.parametrize('W', [50, 64])
def test_four_launch_forms_agree(sample, W):
    """launch by launch | captured (every graph replayed at least twice) | xw_substep_gen / _disc | with reuse_test_net"""
    forms = {'launch by launch': dict(use_graphs=False), 'captured': dict(), 'runner': dict(), 'reuse_test_net': dict(reuse_test_net=True)}
    runs = {}
    for name, extra in forms.items():
        S = _engine(W, **dict(CACHED, **extra))
        G = _load(S, sample)
        if name == 'runner':
            G.persistent = False                    # (what train() sets on the groups of a list domain: eager, through the C runner)
            assert S.engine._runner_ok(G)
        runs[name] = _run(S.engine, G)
        if name == 'captured':
            assert set(G.graphs) == {'gen_xc', 'disc_act_xc'}
    for name in list(forms)[1:]:
        _same(runs['launch by launch'], runs[name], '%s against launch by launch, W = %d' % (name, W))


def _write_phi_in_place(S):
    with torch.no_grad():
        for p_ in S.v_net.parameters():
            p_.mul_(1.25)                           # torch-side write: bumps the parameters' version counters


def _write_phi_unseen(S):
    before = sum(p._version for p in S.engine.phi.params)
    S.engine.phi.data.data.mul_(0.75)               # (.data: a write no version counter of phi sees)
    assert sum(p._version for p in S.engine.phi.params) == before
    S.engine.invalidate_test_net()


@pytest.mark.parametrize('event', ['in_place_write', 'invalidate', 'resample'])
def test_a_stale_table_is_formed_again(sample, event):
    """phi written from outside between sub-steps, invalidate_test_net(), a new sample into the same buffers: each equal to the
    engine that forms the table at every head, given the same events (in front of sub-steps 1 and 3 of g, g, d, g, d)"""
    runs = []
    for opts in (CACHED, AT_HEAD):
        S = _engine(50, **opts)
        G = _load(S, sample)
        ev = {'in_place_write': lambda: _write_phi_in_place(S), 'invalidate': lambda: _write_phi_unseen(S),
              'resample': lambda: _load(S, sample, which=2, into=G)}[event]
        if event == 'resample':
            arena = G._arena.data_ptr()
            runs.append(_run(S.engine, G, between={1: ev, 3: ev}))
            assert G._arena.data_ptr() == arena and G.sample_version == 2
        else:
            runs.append(_run(S.engine, G, between={1: ev, 3: ev}))
    _same(runs[0], runs[1], event)


def _counting(monkeypatch):
    from xnode_wan_pde_solver_amd import kernels as KN
    calls, real = [], KN.disc_xproj

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(KN, 'disc_xproj', counted)
    return calls


def test_table_is_formed_once_per_load_and_once_per_discriminator_substep(sample, monkeypatch):
    calls = _counting(monkeypatch)
    S = _engine(50, **dict(CACHED, use_graphs=False))
    eng = S.engine
    G = _load(S, sample)
    assert len(calls) == 1                                              # the load
    seen = []
    for c in SEQ:
        n0 = len(calls)
        (eng.generator_step if c == 'g' else eng.discriminator_step)(G)
        seen.append(len(calls) - n0)
    assert seen == [0, 0, 1, 0, 1], seen                                # none at a head; one behind each update of phi
    _load(S, sample, which=2, into=G)
    assert len(calls) == 4
    eng.generator_step(G)
    assert len(calls) == 4
    eng.invalidate_test_net()
    eng.generator_step(G)                                               # the key no longer matches: formed at the head, once
    eng.generator_step(G)
    assert len(calls) == 5
    torch.cuda.synchronize()


def test_paths_that_keep_their_launches(sample, monkeypatch):
    """a point-mode group, a tiled-family test network and xproj_cached=False take none of the new launches"""
    calls = _counting(monkeypatch)
    domain, pts = sample[0], sample[1]
    # point mode: the paths of the group do not share one time column -- no table below xproj_min_d, no launch
    S = _engine(50, **dict(CACHED, use_graphs=False))
    XV = pts.interiorv.clone()
    XV[1:, 1, 0] += 0.03125
    G = S.engine.load_group(pts.interioru, XV, pts.boundary, domain)
    assert G.tpp is not None and G.ptr('xproj') == 0 and not S.engine._xproj_held(G)
    _run(S.engine, G, 'gdg')
    assert len(calls) == 0
    # the tiled family hoists nothing
    S = _engine(50, params=_params(50, v_layers=17), **dict(CACHED, use_graphs=False))
    assert S.engine.testnet == 'tiled' and not S.engine.xproj_cached
    G = _load(S, sample)
    assert G.ptr('xproj') == 0
    _run(S.engine, G, 'gdg')
    assert len(calls) == 0
    # caching off: the table at the head of every test-network launch and nowhere else
    S = _engine(50, **dict(AT_HEAD, use_graphs=False))
    G = _load(S, sample)
    assert len(calls) == 0
    _run(S.engine, G, 'ggdg')
    assert len(calls) == 4
    # ... and with neither switch the input layer runs per point at this d
    S = _engine(50, xproj_cached=False, use_graphs=False)
    G = _load(S, sample)
    assert G.ptr('xproj') == 0


@pytest.mark.parametrize('W', [50, 64])
def test_table_in_a_guarded_arena(sample, W):
    """the table launch on guard-banded, poisoned buffers at the group's shapes: guards intact, every element written, rows >= W zero,
    rows < W the input layer's spatial columns"""
    from xnode_wan_pde_solver_amd import kernels as KN
    S = _engine(W, **CACHED)
    G = _load(S, sample)
    eng = S.engine
    torch.cuda.synchronize()
    A = Arena('cuda')
    xT, phi = A.inp(G.xvT, name='xvT'), A.inp(eng.phi.data, name='phi')
    rows = KN.disc_xproj_rows(W)
    xp = A.out(rows, G.N, name='xproj')
    KN.disc_xproj(xT, phi, W, out=xp)
    A.check(written=[xp])
    assert rows == 64 and not bool(xp[W:].ne(0).any())
    assert torch.equal(xp, G.xproj)                                     # what load_group formed
    Vin, b = eng.phi.params[0].detach().double(), eng.phi.params[1].detach().double()
    ref = Vin[:, 1:] @ G.xvT + b.reshape(-1, 1)
    np.testing.assert_allclose(xp[:Vin.shape[0]].cpu().numpy(), ref.cpu().numpy(), rtol=0, atol=64 * 2.0 ** -52 * float(ref.abs().max() + 1))
