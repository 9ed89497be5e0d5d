"""Per-call kernel times from a rocprofv3 kernel trace: calls, mean, min, median and max per kernel, over the calls that
follow the warm-up (the first third of a kernel's calls is dropped).  `expand_kernel`, `sh_colour_listed_kernel` and
`blend_quadrant_kernel` run once per depth slab, so their calls are split into [even] (slab 0) and [odd] (slab 1) for a two-slab frame.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o r -- python bench.py --profile-run --streams 1
    python scripts/kernel_call_stats.py DIR/.../r_kernel_trace.csv out.csv
What profiles/r07_trim_*_kernel_calls.csv were made with (220 calls per launch, the last 147 kept)."""
import collections
import csv
import re
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
per = collections.defaultdict(list)
for r in rows:
    n = re.sub(r'\(anonymous namespace\)::', '', r['Kernel_Name']); n = re.sub(r'^void ', '', n)
    per[n.split('(')[0]].append((int(r['Start_Timestamp']), int(r['End_Timestamp']) - int(r['Start_Timestamp'])))
out = []
for n, v in per.items():
    v.sort()
    d = [x[1] for x in v]
    groups = {'': d}
    if n.startswith(('gsr::expand_kernel', 'gsr::sh_colour_listed_kernel', 'gsr::blend_quadrant_kernel')):
        groups = {'[even]': d[0::2], '[odd]': d[1::2]}
    for g, dd in groups.items():
        dd = dd[len(dd) // 3:]   # drop the warm-up calls
        dd2 = sorted(dd)
        out.append((sum(dd), n + g, len(dd), sum(dd) / len(dd) / 1e3, dd2[0] / 1e3, dd2[len(dd2) // 2] / 1e3, dd2[-1] / 1e3))
out.sort(reverse=True)
with open(sys.argv[2], 'w') as f:
    f.write('kernel,calls,mean_us,min_us,median_us,max_us\n')
    for _, n, c, m, lo, med, hi in out:
        f.write(f'"{n}",{c},{m:.2f},{lo:.2f},{med:.2f},{hi:.2f}\n')
for _, n, c, m, lo, med, hi in out[:16]:
    print(f'{c:5d} mean {m:8.2f} min {lo:8.2f} med {med:8.2f} max {hi:8.2f}  {n[:70]}')
