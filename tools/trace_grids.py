"""Summarise a rocprofv3 kernel trace (`--kernel-trace --output-format csv`, the *_kernel_trace.csv file) by launch geometry: one row
per (kernel, grid in workgroups, workgroup size) with the number of dispatches and their total time.  rocprofv3 reports Grid_Size in
work-items; this divides by the workgroup size.

    python tools/trace_grids.py TRACE.csv [--match REGEX] > grids.csv
"""
import argparse
import collections
import csv
import re
import sys


def summarise(path, match=None):
    rows = collections.OrderedDict()
    pat = re.compile(match) if match else None
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if pat and not pat.search(name):
                continue
            wg = tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ")
            grid = tuple(int(r[f"Grid_Size_{a}"]) // w for a, w in zip("XYZ", wg))
            key = (name, grid, wg)
            n, ns = rows.get(key, (0, 0))
            rows[key] = (n + 1, ns + int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("trace")
    ap.add_argument("--match", default=None, help="keep kernels whose name matches this regular expression")
    a = ap.parse_args(argv)
    w = csv.writer(sys.stdout)
    w.writerow(["Name", "GridWG_X", "GridWG_Y", "GridWG_Z", "Workgroup", "Calls", "TotalDurationNs"])
    for (name, grid, wg), (n, ns) in sorted(summarise(a.trace, a.match).items(), key=lambda kv: (kv[0][0], kv[0][1])):
        w.writerow([name, *grid, "x".join(map(str, wg)), n, ns])


if __name__ == "__main__":
    main()
