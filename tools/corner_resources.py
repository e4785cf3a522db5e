#!/usr/bin/env python3
"""profiles/<tag>_strip_resources.json: registers, scratch, occupancy and LDS of every instantiation of the strip corner
kernel, both responses (k_eig_strip<BS>, k_harris_strip<BS>), from the compiler's resource remarks (hipcc
-Rpass-analysis=kernel-resource-usage on csrc/k_corners.hip as the library builds it).  No GPU needed.
Usage: tools/corner_resources.py [<tag>]     without a tag the figures are only printed"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tag = sys.argv[1] if len(sys.argv) > 1 else None
cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
       "-Rpass-analysis=kernel-resource-usage", "-c", "k_corners.hip", "-o", "/dev/null"]
run = subprocess.run(cmd, cwd=os.path.join(ROOT, "iceberg_tracking_code_amd", "csrc"), capture_output=True, text=True)
if run.returncode != 0:
    sys.exit("hipcc failed (exit %d):\n%s" % (run.returncode, run.stderr[-2000:]))
txt = run.stderr
out, cur = {}, None
for line in txt.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        mm = re.search(r"(k_eig_strip|k_harris_strip)ILi(\d+)E", m.group(1))
        cur = "%s<%s>" % mm.groups() if mm else None
        if cur:
            out[cur] = {}
        continue
    if cur is None:
        continue
    for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch_bytes", r"ScratchSize \[bytes/lane\]: (\d+)"),
                     ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"), ("sgpr_spills", r"SGPRs Spill: (\d+)"),
                     ("vgpr_spills", r"VGPRs Spill: (\d+)"), ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)")):
        m = re.search(pat, line)
        if m:
            out[cur][key] = int(m.group(1))
out = {k: out[k] for k in sorted(out, key=lambda n: (n.split("<")[0], int(n.split("<")[1][:-1])))}
if len(out) != 8:
    sys.exit("expected the remarks of 8 strip kernels, found %d" % len(out))
if tag:
    with open(os.path.join(ROOT, "profiles", "%s_strip_resources.json" % tag), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
print(json.dumps(out, indent=1))
