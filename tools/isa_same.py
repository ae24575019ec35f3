#!/usr/bin/env python3
"""Is the gfx950 device code of two builds the same?  Runs on the CPU (llvm-objdump only).
usage: tools/isa_same.py A B      A, B: two directories of objects (compared by file name) or two libxnwan.so
       tools/isa_same.py --by-kernel A B      for two builds that partition their kernels into objects differently (see below)
Per object: the gfx950 bundle (llvm-objdump --offloading) byte for byte; where the bytes differ, per kernel symbol the instruction
text without addresses, .vgpr_count / .agpr_count / .sgpr_count and the scratch and LDS size of the notes.  One line per object:
'identical' or 'N kernels differ' and their names; exit status 1 on any difference.
--by-kernel: every kernel symbol of A against the same symbol of B, in whichever object (or code object of a library) each sits:
the instruction text up to the symbol's size -- what the disassembler prints for the alignment padding behind a kernel's last
instruction depends on what follows it --, the register counts, scratch and LDS.  Lists the kernels that differ, the kernels
present on one side only, and the objects whose gfx950 bundles are byte-identical; exit status 1 on any of the first two."""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/llvm/bin')
KEYS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def bundles(path, tmp):
    """the extracted gfx950 code objects of `path` in file order: one per object, one per linked object in a library, none if host-only"""
    d = tempfile.mkdtemp(dir=tmp)
    os.symlink(os.path.abspath(path), os.path.join(d, 'in'))
    run(LLVM + '/llvm-objdump', '--offloading', 'in', cwd=d)
    return sorted(glob.glob(os.path.join(d, 'in.*gfx950*')), key=lambda f: int(os.path.basename(f).split('.')[1]))


def kernels(co):
    """{kernel symbol: (instruction lines, {note key: value})}"""
    body, cur = {}, None
    for line in run(LLVM + '/llvm-objdump', '-d', co).splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
        if m:
            cur = body.setdefault(m.group(1), [])
        elif cur is not None and line.startswith('\t'):
            cur.append(re.sub(r'\s*//.*$', '', line).strip())
    out = {}
    for blk in re.split(r'\n  - (?=\.)', run(LLVM + '/llvm-readelf', '--notes', co))[1:]:
        kv = dict(re.findall(r'^    \.(\w+):\s+(\S+)$', blk, re.M))   # (kernel-level keys: four spaces; arguments sit deeper)
        if 'symbol' in kv:
            name = kv['symbol'][:-3] if kv['symbol'].endswith('.kd') else kv['symbol']
            out[name] = (body.get(name), {k: kv.get(k) for k in KEYS})
    return out


def kernels_sized(co):
    """{kernel symbol: (instruction lines below the symbol's end, {note key: value})}: by address, from the symbol table"""
    lines = []
    for line in run(LLVM + '/llvm-objdump', '-d', co).splitlines():
        m = re.match(r'^\t(.*?)\s*// ([0-9A-F]+): ', line)
        if m:
            lines.append((int(m.group(2), 16), m.group(1).strip()))
    span = {}
    for m in re.finditer(r'^\s*\d+: ([0-9a-f]+)\s+(\d+) FUNC\s+\S+\s+\S+\s+\S+ (\S+)$', run(LLVM + '/llvm-readelf', '-sW', co), re.M):
        span[m.group(3)] = (int(m.group(1), 16), int(m.group(1), 16) + int(m.group(2)))
    return {k: ([t for a, t in lines if span[k][0] <= a < span[k][1]] if k in span else None, notes) for k, (_, notes) in kernels(co).items()}


def objects(path):
    return [os.path.join(path, n) for n in sorted(os.listdir(path)) if n.endswith('.o')] if os.path.isdir(path) else [path]


def by_kernel(a, b):
    """compare per kernel symbol over all code objects of A and of B"""
    with tempfile.TemporaryDirectory() as tmp:
        side, raw = [], []
        for root in (a, b):
            ks, bytes_of = {}, {}
            for obj in objects(root):
                cos = bundles(obj, tmp)
                bytes_of[os.path.basename(obj)] = [open(c, 'rb').read() for c in cos]
                for i, c in enumerate(cos):
                    for k, v in kernels_sized(c).items():
                        ks[k] = v + (os.path.basename(obj) + ('[%d]' % i if len(cos) > 1 else ''),)
            side.append(ks)
            raw.append(bytes_of)
    ka, kb = side
    both = sorted(set(ka) & set(kb))
    bad = [k for k in both if ka[k][:2] != kb[k][:2] or ka[k][0] is None]
    moved = [k for k in both if ka[k][2] != kb[k][2]]
    print('%d kernels in A, %d in B, %d in both: %d identical (instructions to the symbol size, registers, scratch, LDS), %d differ; '
          '%d sit in an object of another name' % (len(ka), len(kb), len(both), len(both) - len(bad), len(bad), len(moved)))
    for k in bad:
        print('differs   %s   (%s | %s)' % (k, ka[k][2], kb[k][2]))
    for name, x, y in (('A', ka, kb), ('B', kb, ka)):
        for k in sorted(set(x) - set(y)):
            print('only in %s %s   (%s)' % (name, k, x[k][2]))
    if os.path.isdir(a):
        for n in sorted(set(raw[0]) | set(raw[1])):
            print('%-28s %s' % (n, 'only in A' if n not in raw[1] else 'only in B' if n not in raw[0] else
                                'bundle byte-identical' if raw[0][n] == raw[1][n] else 'bundle bytes differ'))
    return 1 if bad or set(ka) ^ set(kb) else 0


def compare(a, b, tmp):
    ca, cb = bundles(a, tmp), bundles(b, tmp)
    if len(ca) != len(cb):
        return '%d code objects against %d' % (len(ca), len(cb)), True
    differ = [(x, y) for x, y in zip(ca, cb) if open(x, 'rb').read() != open(y, 'rb').read()]
    if not differ:
        return 'identical (%s)' % ('no device code' if not ca else '%d code objects' % len(ca) if len(ca) > 1 else '1 code object'), False
    ka, kb = {}, {}
    for x, y in differ:
        ka.update(kernels(x))
        kb.update(kernels(y))
    bad = sorted(k for k in set(ka) | set(kb) if ka.get(k) != kb.get(k))
    if not bad:
        return '0 kernels differ of %d (instructions, registers, scratch, LDS), the bytes do: symbol placement' % len(ka), True
    return '%d kernels differ: %s' % (len(bad), ' '.join(bad)), True


def main(a, b):
    if os.path.isdir(a):
        pairs = [(n, os.path.join(a, n), os.path.join(b, n)) for n in sorted(os.listdir(a)) if n.endswith('.o')]
        only = sorted(n for n in os.listdir(b) if n.endswith('.o') and not os.path.exists(os.path.join(a, n)))
    else:
        pairs, only = [(os.path.basename(a), a, b)], []
    rc = 0
    with tempfile.TemporaryDirectory() as tmp:
        for n, pa, pb in pairs:
            text, diff = compare(pa, pb, tmp) if os.path.exists(pb) else ('missing in ' + b, True)
            print('%-28s %s' % (n, text))
            rc |= diff
    for n in only:
        print('%-28s missing in %s' % (n, a))
    return 1 if rc or only else 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--by-kernel':
        sys.exit(by_kernel(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
