#!/usr/bin/env python3
"""rocprofv3 --kernel-trace csv -> a markdown table like kernel_stats_md.py's, with the launches of the kernels named by
--split listed per launch shape (grid x workgroup) instead of summed: one row per shape, in launch order.
usage: kernel_trace_md.py run_kernel_trace.csv STEPS_TRACED 'title' [--split substr ...] > profiles/<tag>_kernel_stats.md"""
import csv, sys

args = sys.argv[1:]
split = []
if "--split" in args:
    i = args.index("--split")
    split, args = args[i + 1:], args[:i]
src, steps, title = args[0], int(args[1]), args[2]
rows, order = {}, []
for r in csv.DictReader(open(src)):
    name = r["Kernel_Name"]
    key = (name, "")
    if any(s in name for s in split):
        wg = [int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"]
        key = (name, " grid " + "x".join(str(int(r[f"Grid_Size_{a}"]) // w) for a, w in zip("XYZ", wg) if int(r[f"Grid_Size_{a}"]) // w > 1 or a == "X"))
    if key not in rows:
        rows[key] = [0, 0.0]
        order.append(key)
    rows[key][0] += 1
    rows[key][1] += float(r["End_Timestamp"]) - float(r["Start_Timestamp"])
tot = sum(v[1] for v in rows.values())
print(f"# {title}\n\n{steps} steps traced; kernel time {tot / steps / 1e6:.2f} ms per step.\n")
print("| kernel | calls | ms/step | avg us | % |\n|---|---|---|---|---|")
for key in sorted(order, key=lambda k: -rows[k][1])[:44]:
    n, t = rows[key]
    short = key[0].replace("s2vt::(anonymous namespace)::", "s2vt::")[:90]
    print(f"| `{short}`{key[1]} | {n} | {t / steps / 1e6:.3f} | {t / n / 1e3:.1f} | {100 * t / tot:.1f} |")
