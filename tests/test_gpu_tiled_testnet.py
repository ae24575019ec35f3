"""The tiled test-network family (csrc/xw_disc_tiled.hip) against the oracle under autograd: forward, time tangent, fused input
gradient, record and reverse at widths and depths only it serves, the tiled family against the MFMA containers at their widths,
bitwise reproducibility (eager and graph replay) and the C refusals."""
import pytest
import torch

from oracle import refspec as R
from xnode_wan_pde_solver_amd import kernels as KN, _lib

pytestmark = pytest.mark.gpu
F64 = torch.float64
V_ORDER = ['Vin', 'Vin_b', 'Vh', 'Vh_b', 'Vo', 'Vo_b']


def _phi(d, W, q, seed):
    cfg = {'alpha': 1e8, 'u_layers': 2, 'u_hidden_dim': 20, 'u_hidden_hidden_dim': 10, 'v_layers': q, 'v_hidden_dim': W,
           'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'midpoint'}
    setup = {'dim': d, 'N_t': 2, 'N_r': 1, 'N_b': 1, 'T0': 0, 'T': 1, 'shape_param': [-1, 1]}
    torch.manual_seed(seed)
    _, phi = R.init_parameters(cfg, setup)
    for p_ in phi.values():
        if p_.dim() == 1:
            p_.copy_(0.3 * torch.randn_like(p_))
    return cfg, phi


def _sample(N, L, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, d, generator=g, dtype=F64) * 2 - 1
    t, _ = torch.sort(torch.rand(L, generator=g, dtype=F64))
    t[0] = 0.0
    X = torch.cat((t.view(1, L, 1).expand(N, L, 1), x.view(N, 1, d).expand(N, L, d)), 2).contiguous()
    return x, t, X


def _close(a, b, tol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(float(b.abs().max()), 1e-300)
    err = float((a - b).abs().max()) / scale
    assert err < tol, '%s: max rel-to-scale error %.3e (scale %.3e)' % (what, err, scale)


def _blob(phi):
    return torch.cat([phi[k].reshape(-1) for k in V_ORDER]).cuda()


def _reference(phi, cfg, X, vbar, q):
    ph = {k: v.clone().requires_grad_(True) for k, v in phi.items()}
    Xd = X.clone().requires_grad_(True)
    v = R.v_net(ph, cfg, Xd)
    used = [k for k in V_ORDER if q > 0 or not k.startswith('Vh')]
    grads = dict(zip(used, torch.autograd.grad((v * vbar).sum(), [ph[k] for k in used], retain_graph=True)))
    gX = torch.autograd.grad(v.sum(), Xd)[0]
    gphi = torch.cat([(grads[k] if k in grads else torch.zeros_like(phi[k])).reshape(-1) for k in V_ORDER])
    return v.detach(), gX, gphi


# (W, q, d, N, L): N L never a multiple of 16 or 64
CASES = [(129, 0, 5, 37, 3), (129, 17, 20, 21, 5), (200, 1, 1, 45, 3), (200, 9, 100, 19, 4), (256, 9, 20, 29, 5),
         (256, 32, 5, 13, 3), (256, 17, 1, 23, 3), (160, 20, 100, 11, 7), (64, 20, 5, 27, 3), (100, 32, 20, 9, 9)]


@pytest.mark.parametrize('W,q,d,N,L', CASES)
def test_tiled_path_mode_matches_the_oracle(W, q, d, N, L):
    assert KN.testnet_family(W, q) == 'tiled'
    cfg, phi = _phi(d, W, q, 71 + W + q)
    x, t, X = _sample(N, L, d, 72 + d)
    vbar = torch.randn(N, L, dtype=F64, generator=torch.Generator().manual_seed(73))
    v_ref, gX, gphi = _reference(phi, cfg, X, vbar, q)
    xT, tc, blob = x.t().contiguous().cuda(), t.cuda(), _blob(phi)
    act = torch.full((KN.disc_act_rows(W, q), KN.disc_act_cols(N * L)), float('nan'), dtype=F64, device='cuda')
    gxv = torch.empty(d, N, dtype=F64, device='cuda')
    gtv = torch.empty(N, dtype=F64, device='cuda')
    v, vt = KN.disc_fwd(xT, tc, blob, W, q, gxv=gxv, gtv=gtv, ngrad=N, act=act)
    _close(v.t(), v_ref, 1e-12, 'v')
    _close(vt.t(), gX[:, :, 0], 1e-11, 'dv/dt')
    _close(gxv.t(), gX[:, 0, 1:], 1e-11, 'nabla_x v')
    _close(gtv, gX[:, 0, 0], 1e-11, 'dv/dt (reverse) at t0')
    vb = vbar.t().contiguous().cuda()
    got = KN.slab_sum(KN.disc_bwd(xT, tc, blob, vb, W, q, act=act)).cpu()
    _close(got, gphi, 1e-10, 'phi gradient (record)')
    got2 = KN.slab_sum(KN.disc_bwd(xT, tc, blob, vb, W, q)).cpu()        # (the wrapper stores a record first)
    assert torch.equal(got, got2)


@pytest.mark.parametrize('W,q,d,N', [(256, 9, 20, 77), (129, 17, 5, 13), (192, 32, 100, 40), (256, 0, 3, 5)])
def test_tiled_point_mode_and_module_surface_match_the_oracle(W, q, d, N):
    cfg, phi = _phi(d, W, q, 81 + q)
    g = torch.Generator().manual_seed(82)
    X = torch.cat((torch.rand(N, 1, generator=g, dtype=F64), torch.rand(N, d, generator=g, dtype=F64) * 2 - 1), 1)
    vbar = torch.randn(N, dtype=F64, generator=g)
    v_ref, gX, gphi = _reference(phi, cfg, X, vbar, q)
    xT, tpp, blob = X[:, 1:].t().contiguous().cuda(), X[:, 0].contiguous().cuda(), _blob(phi)
    v, vt = KN.disc_fwd(xT, None, blob, W, q, tpp=tpp)
    _close(v[0], v_ref, 1e-12, 'v')
    _close(vt[0], gX[:, 0], 1e-11, 'dv/dt')
    gxv, gtv = KN.disc_gradx(xT, None, blob, W, q, tpp=tpp, vbar=vbar.cuda())
    _close(gxv.t(), gX[:, 1:] * vbar[:, None], 1e-11, 'nabla_x v')
    _close(gtv, gX[:, 0] * vbar, 1e-11, 'dv/dt (reverse)')
    got = KN.slab_sum(KN.disc_bwd(xT, None, blob, vbar.view(1, -1).cuda(), W, q, tpp=tpp)).cpu()
    _close(got, gphi, 1e-10, 'phi gradient')
    # the module surface: v_net(XV) and .backward() through the custom operators
    # (at v_layers = 0 the unused hidden Linear stays outside TestNet.net and keeps float32: not bindable, as before)
    if q == 0:
        return
    from xnode_wan_pde_solver_amd import nets
    net = nets.TestNet(cfg, {'dim': d})
    with torch.no_grad():
        net.input.weight.copy_(phi['Vin']); net.input.bias.copy_(phi['Vin_b'])
        net.hidden.weight.copy_(phi['Vh']); net.hidden.bias.copy_(phi['Vh_b'])
        net.output.weight.copy_(phi['Vo']); net.output.bias.copy_(phi['Vo_b'])
    net.bind(torch.device('cuda'))
    assert net.family == 'tiled' and net.kwidth == W
    XV = X.cuda().requires_grad_(True)
    out = net(XV)
    _close(out[:, 0], v_ref, 1e-12, 'module v')
    (out[:, 0] * vbar.cuda()).sum().backward()
    _close(XV.grad, gX * vbar[:, None], 1e-11, 'module input gradient')
    gm = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).cpu()
    _close(gm, gphi, 1e-10, 'module phi gradient')


@pytest.mark.parametrize('W', [50, 64, 96, 128])
def test_tiled_family_agrees_with_the_containers(W):
    q, d, N, L = 9, 20, 45, 3
    cfg, phi = _phi(d, W, q, 90 + W)
    x, t, X = _sample(N, L, d, 91)
    vbar = torch.randn(L, N, dtype=F64, generator=torch.Generator().manual_seed(92)).cuda()
    xT, tc, blob = x.t().contiguous().cuda(), t.cuda(), _blob(phi)
    out = {}
    for fam in ('mfma', 'tiled'):
        gxv = torch.empty(d, N, dtype=F64, device='cuda')
        gtv = torch.empty(N, dtype=F64, device='cuda')
        v, vt = KN.disc_fwd(xT, tc, blob, W, q, gxv=gxv, gtv=gtv, ngrad=N, family=fam)
        gp = KN.slab_sum(KN.disc_bwd(xT, tc, blob, vbar, W, q, family=fam))
        out[fam] = (v, vt, gxv, gtv, gp)
    for i, (name, tol) in enumerate((('v', 1e-12), ('dv/dt', 1e-11), ('nabla_x v', 1e-11), ('dv/dt at t0', 1e-11),
                                     ('phi gradient', 1e-10))):
        _close(out['tiled'][i], out['mfma'][i], tol, name)


def test_tiled_results_are_bitwise_reproducible_eager_and_replayed():
    W, q, d, N, L = 256, 9, 20, 300, 8
    _, phi = _phi(d, W, q, 95)
    x, t, _ = _sample(N, L, d, 96)
    xT, tc, blob = x.t().contiguous().cuda(), t.cuda(), _blob(phi)
    vbar = torch.randn(L, N, dtype=F64, generator=torch.Generator().manual_seed(97)).cuda()
    v = torch.empty(L, N, dtype=F64, device='cuda')
    vt = torch.empty_like(v)
    gxv = torch.empty(d, N, dtype=F64, device='cuda')
    gtv = torch.empty(N, dtype=F64, device='cuda')
    act = torch.empty(KN.disc_act_rows(W, q), KN.disc_act_cols(N * L), dtype=F64, device='cuda')
    slab = torch.empty(KN.disc_bwd_slabs(N, L), blob.numel(), dtype=F64, device='cuda')

    def run():
        KN.disc_fwd(xT, tc, blob, W, q, v=v, vt=vt, gxv=gxv, gtv=gtv, ngrad=N, act=act, max_blocks=7)
        KN.disc_bwd(xT, tc, blob, vbar, W, q, gslab=slab, act=act)

    def snap():
        return [b.clone() for b in (v, vt, gxv, gtv, slab)]

    run()
    first = snap()
    run()
    for a, b in zip(first, snap()):
        assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for _ in range(2):
        for b in (v, vt, gxv, gtv, slab):
            b.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, snap()):
            assert torch.equal(a, b)


def test_tiled_c_refusals():
    L_ = _lib.lib
    p = KN._p
    d, N, L = 5, 16, 2
    xT = torch.zeros(d, N, dtype=F64, device='cuda')
    t = torch.zeros(L, dtype=F64, device='cuda')
    v = torch.zeros(L, N, dtype=F64, device='cuda')
    phi = torch.zeros(KN.phi_size(d, 256), dtype=F64, device='cuda')
    slab = torch.zeros(KN.disc_bwd_slabs(N, L), phi.numel(), dtype=F64, device='cuda')
    act = torch.zeros(KN.disc_act_rows(256, 9), KN.disc_act_cols(N * L), dtype=F64, device='cuda')
    fwd = lambda W, q, d_=d, xproj=None, xT_=xT, gxv=None, ngrad=0: L_.xw_disc_tiled_fwd(   # noqa: E731
        p(xT_), p(t), None, p(phi), N, L, d_, W, q, p(v), None, p(gxv), None, ngrad, 0, None, p(xproj), None)
    bwd = lambda W, q, a=act, d_=d: L_.xw_disc_tiled_bwd(p(xT), p(t), None, p(phi), None, N, L, d_, W, q, p(a), p(slab), None)  # noqa: E731
    assert fwd(257, 9) == -1 and fwd(256, 33) == -1 and fwd(256, 9, d_=127) == -1
    assert bwd(257, 9) == -1 and bwd(256, 33) == -1 and bwd(256, 9, d_=127) == -1
    assert bwd(256, 9, a=None) == -1                                   # (from the record only)
    assert fwd(256, 9, xproj=v) == -2                                  # (no x-projection table)
    assert fwd(256, 9, xT_=None) == -2
    assert fwd(256, 9, gxv=xT, ngrad=N * L + 1) == -2
    assert L_.xw_disc_tiled_bwd(p(xT), p(t), None, p(phi), None, N, L, d, 256, 9, p(act), None, None) == -2
    torch.cuda.synchronize()
