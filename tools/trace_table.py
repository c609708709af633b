"""Per-kernel table of a rocprofv3 --kernel-trace run of bench.py (the rocpd database rocprofv3 writes): launches and GPU time per
frame.  python tools/trace_table.py <results.db> <frames>     (frames = (steps + warmup) x clips of the traced run)"""
import collections
import re
import sqlite3
import sys

db, frames = sys.argv[1], float(sys.argv[2])
rows = sqlite3.connect(db).execute("select name, duration from kernels").fetchall()
agg = collections.OrderedDict()
for name, dur in rows:
    short = re.sub(r"\(.*", "", name.replace("void ", "").replace("vbt::", ""))
    short = re.sub(r"<.*", "", short)
    a = agg.setdefault(short, [0, 0])
    a[0] += 1
    a[1] += dur
tot_n, tot_t = sum(a[0] for a in agg.values()), sum(a[1] for a in agg.values())
print("| kernel | launches | launches / frame | us / launch | us / frame | share |\n|---|---:|---:|---:|---:|---:|")
for k, (n, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
    print(f"| {k} | {n} | {n / frames:.4f} | {t / n / 1e3:.1f} | {t / frames / 1e3:.3f} | {100 * t / tot_t:.1f} % |")
print(f"| total | {tot_n} | {tot_n / frames:.4f} | {tot_t / tot_n / 1e3:.1f} | {tot_t / frames / 1e3:.3f} | 100 % |")
