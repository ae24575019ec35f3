#!/usr/bin/env python3
"""Reference fixtures for the tiled test-network family (csrc/xw_disc_tiled.hip): test networks wider than 128 and deeper than 16.

Usage:  python tests/golden/make_golden_wide_testnet.py      (needs the reference, as make_golden.py; CPU, a few minutes)

Runs the reference's own code through make_golden.py's one_iteration / trajectory (that file is imported, not changed):
    ref_wide_testnet_d4_midpoint     one outer iteration, u (20, 10, 8) + v (256, 9), midpoint
    ref_wide_testnet_d3_rk4          one outer iteration, u (48, 16, 4) + v (160, 20), rk4
    ref_wide_testnet_both_d5_euler   one outer iteration, u (128, 32, 4) + v (192, 3), euler: both tiled families together
    ref_traj_wide_testnet_d3_seed50  25 outer iterations of the reference's train(), u (20, 10, 8) + v (256, 9), d = 3

The wide parameter matrices would make the one-iteration files several MB, so each file is compacted after it is written
(`compact`): a parameter array of more than BIG entries is kept as
    <net>_sd_sha1/<name>   the SHA-1 of the reference's initial float64 values (the consumer takes the values from its own
                           solver, built with the same seed, and checks them against this hash: the same exact pin),
    <step>/grad/<name>     the reference's gradient, rounded to float32 (compared at rtol 1e-5),
    <step>/step/<name>     after - before of that optimiser step, float32 (before: the initial values for gen1 / disc1,
                           gen1's result for gen2); the consumer adds it to before (error ~1e-9 against atol 1e-7).
tests/test_gpu_tiled_testnet_engine.py (`expand`) rebuilds the full file make_golden.py would have written.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import one_iteration, trajectory   # noqa: E402

BIG = 4096
BEFORE = {'gen1': 'u_sd/', 'gen2': 'gen1/after/', 'disc1': 'v_sd/'}


def sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def compact(case):
    path = os.path.join(HERE, case + '.npz')
    z = dict(np.load(path))
    out = {}
    for k, a in z.items():
        big = a.dtype == np.float64 and a.size > BIG
        if big and '_sd/' in k:
            out[k.replace('_sd/', '_sd_sha1/', 1)] = np.array(sha1(a))
        elif big and '/grad/' in k:
            out[k] = a.astype(np.float32)
        elif big and '/after/' in k:
            tag, _, name = k.split('/', 2)
            out[tag + '/step/' + name] = (a - z[BEFORE[tag] + name]).astype(np.float32)
        else:
            out[k] = a
    np.savez_compressed(path, **out)
    print('compacted', path, '%.1f KB' % (os.path.getsize(path) / 1024))


def main():
    one_iteration('ref_wide_testnet_d4_midpoint', 4, 48, 28, 6, 46, 'midpoint', True,
                  net=dict(u_hidden_dim=20, u_hidden_hidden_dim=10, u_layers=8, v_hidden_dim=256, v_layers=9))
    compact('ref_wide_testnet_d4_midpoint')
    one_iteration('ref_wide_testnet_d3_rk4', 3, 36, 20, 5, 47, 'rk4', True,
                  net=dict(u_hidden_dim=48, u_hidden_hidden_dim=16, u_layers=4, v_hidden_dim=160, v_layers=20))
    compact('ref_wide_testnet_d3_rk4')
    one_iteration('ref_wide_testnet_both_d5_euler', 5, 40, 24, 5, 48, 'euler', True,
                  net=dict(u_hidden_dim=128, u_hidden_hidden_dim=32, u_layers=4, v_hidden_dim=192, v_layers=3))
    compact('ref_wide_testnet_both_d5_euler')
    trajectory('ref_traj_wide_testnet_d3_seed50', 3, 64, 40, 8, 50, 25, True,
               net=dict(u_hidden_dim=20, u_hidden_hidden_dim=10, u_layers=8, v_hidden_dim=256, v_layers=9))


if __name__ == '__main__':
    main()
