"""The 35 launches of the HIP UNet front-end from a rocprofv3 --kernel-trace CSV of tools/frontend_time.py: mean duration per
position in the sequence (28 convolutions + 7 pools, in launch order), over every pass the trace holds.
usage: python3 tools/frontend_launches.py <kernel_trace.csv>"""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows
            if "k_conv3x3" in r["Kernel_Name"] or "k_adaptive_max_pool" in r["Kernel_Name"])
N = 35
passes = len(ev) // N
assert passes >= 1 and len(ev) % N == 0, f"{len(ev)} front-end launches: not a multiple of {N}"
short = lambda n: "pool" if "max_pool" in n else ("deep" if "deep" in n else ("tile<8>" if "Li8" in n or "<8>" in n else "tile<4>"))
total = 0.0
print(f"{passes} passes of {N} launches")
for k in range(N):
    names = {short(ev[p * N + k][2]) for p in range(passes)}
    assert len(names) == 1, (k, names)
    us = sum(ev[p * N + k][1] - ev[p * N + k][0] for p in range(passes)) / passes / 1e3
    total += us
    print(f"{k:2d}  {names.pop():8s} {us:8.2f} us")
print(f"sum of the {N} kernels: {total:.1f} us")
