#!/usr/bin/env python3
"""dev tool: did two runs launch the same kernels?  (runs here, on the CSVs)

    python tools/ktrace_diff.py DIR_A DIR_B [--symbols names.txt]

DIR_x: output of `rocprofv3 --kernel-trace -d DIR_x -- <program>` (nothing else traced), one *_kernel_trace.csv per process.
Compares, process by process in the order the processes started, the ORDERED sequence of (kernel name, grid size, workgroup
size, LDS bytes).  A program that runs for a TIME (bench.py's sustained rotation) launches another number of steps in every
run: give it a fixed amount of work (`bench.py --sustain 0`).  `--symbols`: a file of kernel names, one per line (demangled,
as the trace prints them); lists those that neither run launched.  Exit status 1 unless every sequence is equal.
"""
import csv, glob, os, sys


def launches(d):
    runs = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Dispatch_Id"]))
        key = lambda r: (r["Kernel_Name"],) + tuple(int(r[c + a]) for c in ("Grid_Size_", "Workgroup_Size_") for a in "XYZ") + (int(r["LDS_Block_Size"]),)
        if rows:
            runs.append((min(int(r["Start_Timestamp"]) for r in rows), [key(r) for r in rows]))
    return [seq for _, seq in sorted(runs, key=lambda t: t[0])]


a, b = launches(sys.argv[1]), launches(sys.argv[2])
bad = len(a) != len(b)
print(f"{len(a)} / {len(b)} processes with launches")
for k, (sa, sb) in enumerate(zip(a, b)):
    first = next((i for i, (x, y) in enumerate(zip(sa, sb)) if x != y), None if len(sa) == len(sb) else min(len(sa), len(sb)))
    same_set = set(sa) == set(sb)
    print(f"process {k}: {len(sa)} / {len(sb)} launches, {len(set(sa))} distinct: " +
          ("equal sequences" if first is None else f"DIFFER at launch {first} (the distinct launches are {'the same' if same_set else 'DIFFERENT'})"))
    if first is not None:
        bad = True
        for s in (sa, sb):
            print("   ", s[first] if first < len(s) else "(end)")
if "--symbols" in sys.argv:
    seen = {r[0] for s in a + b for r in s}
    for name in open(sys.argv[sys.argv.index("--symbols") + 1]).read().splitlines():
        if name and name not in seen:
            print("never launched:", name)
sys.exit(1 if bad else 0)
