"""CPU-side checks of the tiled test-network family (csrc/xw_disc_tiled.hip): which family serves which test network, the refusal
beyond its limits, the C-ABI declarations against the ctypes mirror, and a 256-wide TestNet bound on the CPU.  No kernel is
launched."""
import itertools
import os
import re

import pytest
import torch

from xnode_wan_pde_solver_amd import kernels as KN, nets, _lib
from xnode_wan_pde_solver_amd._lib import XnwanError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('xw_disc_tiled_ok', 'xw_disc_tiled_act_rows', 'xw_disc_tiled_fwd', 'xw_disc_tiled_bwd')


def test_served_test_networks_keep_their_family_and_container():
    for W, q in itertools.product(range(1, 129), range(0, 17)):
        assert KN.testnet_family(W, q) == 'mfma', (W, q)
        assert KN.testnet_kwidth(W, q) == KN.disc_container(W), (W, q)


def test_wider_or_deeper_test_networks_take_the_tiled_family():
    for W, q in itertools.product(list(range(129, 257)) + [1, 50, 64, 100, 128], (0, 1, 9, 16, 17, 20, 32)):
        if W <= 128 and q <= 16:
            continue
        assert KN.testnet_family(W, q) == 'tiled', (W, q)
        assert KN.testnet_kwidth(W, q) == W
        assert _lib.lib.xw_disc_tiled_ok(20, W, q) == 1
        assert _lib.lib.xw_disc_tiled_act_rows(W, q) == (q + 1) * W
    assert KN.disc_act_rows(256, 9) == 2560
    assert KN.disc_act_rows(50, 9, family='tiled') == 500


@pytest.mark.parametrize('W,q', [(257, 9), (300, 1), (128, 33), (256, 40), (0, 9), (64, -1)])
def test_beyond_the_tiled_limits_raises_naming_them(W, q):
    with pytest.raises(XnwanError) as e:
        KN.testnet_family(W, q)
    msg = str(e.value)
    assert 'v_hidden_dim = %d' % W in msg and 'v_layers = %d' % q in msg
    for limit in ('128', '256', '16', '32'):
        assert limit in msg
    assert _lib.lib.xw_disc_tiled_ok(20, W, q) == 0
    assert _lib.lib.xw_disc_tiled_act_rows(W, q) == -1


def test_tiled_ok_refuses_wide_inputs():
    assert _lib.lib.xw_disc_tiled_ok(126, 256, 32) == 1
    assert _lib.lib.xw_disc_tiled_ok(127, 256, 32) == 0
    assert _lib.lib.xw_disc_tiled_ok(0, 256, 9) == 0


def test_family_override_is_checked():
    with pytest.raises(XnwanError, match='family'):
        KN.disc_act_rows(64, 9, family='vector')


def test_tiled_testnet_declarations_match_the_ctypes_mirror():
    hdr = open(os.path.join(ROOT, 'include', 'xnwan.h')).read()
    declared = set(re.findall(r'^\s*int\s+(xw_disc_tiled_\w+)\s*\(', hdr, flags=re.M))
    assert declared == set(NAMES)
    for name in NAMES:
        args = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')
        assert len(args) == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.lib, name)
    assert _lib.ABI_VERSION == 33 == _lib.lib.xw_abi_version()
    buf = (__import__('ctypes').c_char * 1024)()
    _lib.lib.xw_supported_dims(buf, 1024)
    assert b'W<=256' in buf.value and b'q<=32' in buf.value


@pytest.mark.parametrize('W,q,d', [(256, 9, 5), (200, 20, 3), (128, 17, 4)])
def test_wide_testnet_binds_on_the_cpu(W, q, d):
    cfg = {'v_layers': q, 'v_hidden_dim': W}
    torch.manual_seed(3)
    net = nets.TestNet(cfg, {'dim': d})
    blob = net.bind(torch.device('cpu'))
    assert net.family == 'tiled' and net.kwidth == W
    assert blob.data.numel() == KN.phi_size(d, W)
    assert torch.equal(blob.data, torch.cat([p.detach().reshape(-1) for p in net.parameters()]))


def test_container_testnet_binds_as_before():
    torch.manual_seed(3)
    net = nets.TestNet({'v_layers': 9, 'v_hidden_dim': 50}, {'dim': 4})
    net.bind(torch.device('cpu'))
    assert net.family == 'mfma' and net.kwidth == 50
