#!/usr/bin/env python3
"""Compile spc_hip.hip with -Rpass-analysis=kernel-resource-usage and print one line per kernel
(VGPRs, SGPRs, spills, scratch, occupancy, LDS).  usage: tools/resusage.py [filter-substring | entry] [extra hipcc flags...]
An entry of ENTRIES names a kernel family that must use no scratch and spill nothing in any instantiation: its lines are
printed and the exit status is 1 if one of them does (tools/resusage.py microphysics, tools/resusage.py diffuse,
tools/resusage.py advect, tools/resusage.py vadvect, tools/resusage.py radiate, tools/resusage.py qtlocal, tools/resusage.py moments, tools/resusage.py transport, tools/resusage.py transport2, tools/resusage.py eddy, tools/resusage.py hmix, tools/resusage.py speed, tools/resusage.py vmix, tools/resusage.py hline)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# K14, K15, K16, K17, K18, K19, K20, K22, K23, K24 (eddy, hmix), K25 (speed, vmix), K26 (hline): every instantiation without scratch and without spills
ENTRIES = {"microphysics": "k_les_microphysics", "diffuse": "k_les_diffuse", "advect": "k_les_advect", "vadvect": "k_les_vadvect",
           "radiate": "k_les_radiate", "qtlocal": "k_les_qt_local", "moments": "k_les_moments", "transport": "k_les_transport", "transport2": "k_les_transport2",
           "eddy": "k_les_eddy", "hmix": "k_les_hmix", "speed": "k_les_speed", "vmix": "k_les_vmix", "hline": "k_les_hline"}
entry = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] in ENTRIES else None
flt = ENTRIES[entry] if entry else sys.argv[1] if len(sys.argv) > 1 else ""
extra = sys.argv[2:]
cmd = ["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
       "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "sp_coupler_amd/csrc/spc_hip.hip"), "-o", "/tmp/resusage.so",
       "-Rpass-analysis=kernel-resource-usage"] + extra
err = subprocess.run(cmd, capture_output=True, text=True).stderr
cur = None
rows = {}
for line in err.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        cur = re.sub(r"\(anonymous namespace\)::", "", cur).split("(")[0].replace("void ", "")
        rows[cur] = {}
        continue
    m = re.search(r"remark:\s+(\w[\w \[\]/]*?): (\d+)", line)
    if m and cur:
        rows[cur][m.group(1).strip()] = int(m.group(2))
bad = []
for name, r in rows.items():
    if flt in name:
        if entry and (r.get("ScratchSize [bytes/lane]", 0) or r.get("SGPRs Spill", 0) or r.get("VGPRs Spill", 0)):
            bad.append(name)
        print("%-62s VGPR %3d AGPR %3d SGPR %3d spillS %3d spillV %3d scratch %4d occ %2d LDS %6d" % (
            name[:62], r.get("VGPRs", -1), r.get("AGPRs", 0), r.get("TotalSGPRs", r.get("SGPRs", -1)), r.get("SGPRs Spill", 0),
            r.get("VGPRs Spill", 0), r.get("ScratchSize [bytes/lane]", 0), r.get("Occupancy [waves/SIMD]", -1),
            r.get("LDS Size [bytes/block]", 0)))
if entry:
    shown = [n for n in rows if flt in n]
    print("%s: %d instantiation(s), %s" % (entry, len(shown), "scratch or spills in %s" % bad if bad else "no scratch, no spill"))
    sys.exit(1 if bad or not shown else 0)
