"""where the x-projection table sits in the g,g,d cycle, from a rocprofv3 kernel trace of tools/cycle_only.py:
    rocprofv3 --kernel-trace --output-format csv -d out -- python3 tools/cycle_only.py 12
    python tools/xproj_trace.py out/*/*_kernel_trace.csv [cycles from the end, default 6] [trimmed.csv]
Per sub-step of the last cycles: its length (first kernel start to last kernel end), the test network's launch (k_disc_fwd without /
with the record), the table kernel (k_disc_xproj) and whether it runs at the HEAD (in front of k_disc_fwd) or BEHIND the update of
phi (k_adam), and the gap between the end of a sub-step's k_adam and the start of the next launch.  Medians over the cycles at the
end; the rows it used go to the trimmed csv (name, queue, start and end in ns from the first row)."""
import csv
import re
import sys

rows = [r for r in csv.DictReader(open(sys.argv[1])) if re.search(r'\bk_\w+', r['Kernel_Name'])]
rows.sort(key=lambda r: int(r['Start_Timestamp']))
cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 6
K = [dict(name=re.search(r'(k_\w+)(<[^>]*>)?', r['Kernel_Name']).group(0), base=re.search(r'k_\w+', r['Kernel_Name']).group(0),
          s=int(r['Start_Timestamp']), e=int(r['End_Timestamp']), q=r['Queue_Id']) for r in rows]
# a sub-step ends with its k_adam -- and with the table kernel when that is the next launch and sits closer to that k_adam than to
# the k_disc_fwd behind it (the hop between two sub-step graphs lies on the other side: formed behind the update of phi, not at a head)
subs, cur, i = [], [], 0
while i < len(K):
    k = K[i]
    cur.append(k)
    if k['base'] == 'k_adam':
        nxt = K[i + 1] if i + 1 < len(K) else None
        if nxt is not None and nxt['base'] == 'k_disc_xproj':
            fwd = next((f for f in K[i + 2:] if f['base'] == 'k_disc_fwd'), None)
            if fwd is None or nxt['s'] - k['e'] < fwd['s'] - nxt['e']:
                cur.append(nxt)
                i += 1
        subs.append(cur)
        cur = []
    i += 1
subs = [s for s in subs if any(k['base'] == 'k_disc_fwd' for k in s)]
subs = subs[-3 * cycles:]
while subs and any(k['base'] in ('k_disc_rec', 'k_disc_bwd') for k in subs[0]):      # start at a generator sub-step
    subs = subs[1:]
med = lambda a: sorted(a)[len(a) // 2] if a else float('nan')  # noqa: E731
us = lambda ns: ns / 1e3  # noqa: E731
stat = {}
prev_adam_end = None
print('%-5s %9s %12s %12s %-7s %10s' % ('kind', 'length', 'k_disc_fwd', 'k_disc_xproj', 'where', 'gap'))
for s in subs:
    kind = 'disc' if any(k['base'] in ('k_disc_rec', 'k_disc_bwd') for k in s) else 'gen'
    first = min(k['s'] for k in s)
    last = max(k['e'] for k in s)
    fwd = next(k for k in s if k['base'] == 'k_disc_fwd')
    tabs = [k for k in s if k['base'] == 'k_disc_xproj']
    where = ','.join('head' if k['s'] < fwd['s'] else 'behind' for k in tabs) or '-'
    adam = [k for k in s if k['base'] == 'k_adam'][-1]
    gap = us(first - prev_adam_end) if prev_adam_end is not None else float('nan')
    prev_adam_end = max(adam['e'], max([k['e'] for k in tabs if k['s'] > adam['s']] or [0]))
    tab_us = sum(us(k['e'] - k['s']) for k in tabs)
    print('%-5s %9.1f %12.1f %12.1f %-7s %10.1f   %s' % (kind, us(last - first), us(fwd['e'] - fwd['s']), tab_us, where, gap, fwd['name'][:40]))
    for key, val in (('length', us(last - first)), ('fwd', us(fwd['e'] - fwd['s'])), ('table', tab_us), ('gap', gap)):
        if val == val:
            stat.setdefault((kind, key), []).append(val)
    stat.setdefault((kind, 'head'), []).append(where.count('head'))
    stat.setdefault((kind, 'behind'), []).append(where.count('behind'))
print()
for kind in ('gen', 'disc'):
    n = len(stat.get((kind, 'length'), []))
    print('%-4s sub-steps %3d: median length %7.1f us   k_disc_fwd %6.1f us   table %4.1f us   gap in front %5.1f us   table launches at the head '
          '%d, behind k_adam %d' % (kind, n, med(stat.get((kind, 'length'), [])), med(stat.get((kind, 'fwd'), [])),
                                    med(stat.get((kind, 'table'), [])), med(stat.get((kind, 'gap'), [])), sum(stat.get((kind, 'head'), [])),
                                    sum(stat.get((kind, 'behind'), []))))
ncyc = len(stat.get(('disc', 'length'), []))
if ncyc:
    cyc = (sum(stat[('gen', 'length')]) + sum(stat[('disc', 'length')]) + sum(stat.get(('gen', 'gap'), [])) + sum(stat.get(('disc', 'gap'), []))) / ncyc
    print('cycle (lengths + gaps) %.1f us over %d cycles; table launches per cycle %.2f' % (
        cyc, ncyc, (sum(stat[('gen', 'head')]) + sum(stat[('gen', 'behind')]) + sum(stat[('disc', 'head')]) + sum(stat[('disc', 'behind')])) / ncyc))
if len(sys.argv) > 3:
    t0 = min(k['s'] for s in subs for k in s)
    with open(sys.argv[3], 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['kernel', 'queue', 'start_ns', 'end_ns'])
        for s in subs:
            for k in s:
                w.writerow([k['name'], k['q'], k['s'] - t0, k['e'] - t0])
