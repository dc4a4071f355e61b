"""Summarise a rocprofv3 kernel trace (`--kernel-trace --output-format csv`, the *_kernel_trace.csv file) by launch geometry: one row
per (kernel, grid in workgroups, workgroup size) with the number of dispatches and their total time.  rocprofv3 reports Grid_Size in
work-items; this divides by the workgroup size.

    python tools/trace_grids.py TRACE.csv [--match REGEX] > grids.csv
    python tools/trace_grids.py TRACE.csv --ordered > launches.csv    (one row per dispatch, in dispatch order, without times:
                                                                       two trees issue the same launches iff these files are equal)
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


def _no_params(name):
    """The kernel's name and template arguments without its parameter list (the trailing parenthesis group)."""
    if not name.endswith(")"):
        return name
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0:
            return name[:i]
    return name


def ordered(path, match=None):
    pat = re.compile(match) if match else None
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if not pat or pat.search(r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    for r in rows:
        wg = tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ")
        yield [_no_params(r["Kernel_Name"]), *(int(r[f"Grid_Size_{a}"]) // w for a, w in zip("XYZ", wg)), "x".join(map(str, wg))]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("trace")
    ap.add_argument("--match", default=None, help="keep kernels whose name matches this regular expression")
    ap.add_argument("--ordered", action="store_true", help="one row per dispatch in dispatch order instead of the summary")
    a = ap.parse_args(argv)
    w = csv.writer(sys.stdout)
    if a.ordered:
        w.writerow(["Name", "GridWG_X", "GridWG_Y", "GridWG_Z", "Workgroup"])
        w.writerows(ordered(a.trace, a.match))
        return
    w.writerow(["Name", "GridWG_X", "GridWG_Y", "GridWG_Z", "Workgroup", "Calls", "TotalDurationNs"])
    for (name, grid, wg), (n, ns) in sorted(summarise(a.trace, a.match).items(), key=lambda kv: (kv[0][0], kv[0][1])):
        w.writerow([name, *grid, "x".join(map(str, wg)), n, ns])


if __name__ == "__main__":
    main()
