#!/usr/bin/env python3
"""Which fused-stepper (or, with --testnet, test-network) kernels did a traced run execute?  Runs on the CPU.
usage: tools/inventory_trace.py [--testnet] LIB STATS.csv [STATS.csv ...]
LIB: a built libxnwan.so (or a directory of xw_ode_*.o); STATS.csv: the *_kernel_stats.csv files of
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python -m pytest tests/test_gpu_stepper_inventory.py -q
(one per traced process).  Prints, with tests/stepper_inventory.py, the number of compiled stepper kernels, how many of them the
trace holds, and the two differences that must be empty for that test file: compiled - traced (kernels no launch reached) and
traced - reaches (launches the restated dispatch does not predict), per kernel family.  Exit status 1 if either is non-empty.
--testnet: the same with tests/testnet_inventory.py, for a trace of tests/test_gpu_testnet_inventory.py (the two child processes of
that file write statistics files of their own: pass them all)."""
import csv
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import stepper_inventory as SI  # noqa: E402
import testnet_inventory as TI  # noqa: E402


def traced(paths, inv=SI):
    """the kernel tuples of inventory `inv` (stepper_inventory or testnet_inventory) named in the first column of the given
    statistics files"""
    out = set()
    for p in paths:
        with open(p, newline='') as f:
            for rec in csv.reader(f):
                k = inv.parse_kernel(rec[0]) if rec else None
                if k is not None:
                    out.add(k)
    return out


def stepper_label(k):
    """the stepper's k_ode_bwd serves three launch forms: told apart in the counts"""
    return k[0] if k[0] != 'bwd' else ('bwd from the store' if k[6] else 'bwd adjoint' if k[7] else 'bwd recomputing')


def testnet_label(k):
    return k[0]


def by_family(kernels, label):
    n = {}
    for k in kernels:
        n[label(k)] = n.get(label(k), 0) + 1
    return ', '.join('%s %d' % kv for kv in sorted(n.items())) or 'none'


def main(lib, stats, inv=SI, label=stepper_label):
    have, ran, want = inv.compiled(lib), traced(stats, inv), set(inv.reached())
    print('compiled %d (%s)' % (len(have), by_family(have, label)))
    print('traced   %d of them (%s)' % (len(have & ran), by_family(have & ran, label)))
    rc = 0
    for what, diff in (('compiled - traced', have - ran), ('traced - reaches', ran - want)):
        print('%s: %d (%s)' % (what, len(diff), by_family(diff, label)))
        for k in sorted(diff, key=repr):
            print('   ', k)
        rc |= bool(diff)
    return rc


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--testnet']
    if len(args) < 2:
        sys.exit(__doc__)
    sys.exit(main(args[0], args[1:], *((TI, testnet_label) if '--testnet' in sys.argv else (SI, stepper_label))))
