#!/usr/bin/env python3
"""What a store stream with holes costs on this device: builds tools/holed_stream.hip if its program is missing, runs it and
prints the raw timings plus, per skip unit, the median and the spread over the repeats ("unit 0" is the dense stream).
`python tools/time_holed_stream.py [repeats] [launches]`; the output belongs in profiles/held_zeros/."""
import os
import re
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
exe, src = os.path.join(HERE, "holed_stream"), os.path.join(HERE, "holed_stream.hip")
if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", src, "-o", exe], check=True)
out = subprocess.run([exe] + sys.argv[1:3], capture_output=True, text=True)
print(out.stdout, end="")
if out.returncode != 0:
    sys.exit(out.stderr)
times = {}
for unit, us in re.findall(r"unit\s+(\d+) B:\s+([\d.]+) us", out.stdout):
    times.setdefault(int(unit), []).append(float(us))
for unit, t in sorted(times.items()):
    print(f"unit {unit:3d} B: median {statistics.median(t):8.2f} us  min {min(t):8.2f}  max {max(t):8.2f}  ({len(t)} repeats)")
