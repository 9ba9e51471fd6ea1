"""global loads / waits per kernel of a `hipcc -S --cuda-device-only` listing (the build's flags): how many vector-memory loads a
kernel holds, how many s_waitcnt wait for ALL of them (vmcnt(0)) and how many allow loads to stay in flight, the longest run of
loads issued back to back before any vmcnt wait, and the VGPR count.   python tools/isa_waits.py file.s [name filter ...]"""
import re
import subprocess
import sys

txt = open(sys.argv[1]).read().split("\n")
flts = sys.argv[2:]
kern = [(i, l.split(":")[0]) for i, l in enumerate(txt) if re.match(r"^_Z\w+:", l)]
dem = subprocess.run(["c++filt"], input="\n".join(n for _, n in kern), capture_output=True, text=True).stdout.split("\n")
print("loads full_waits partial_waits longest_run vgprs kernel")
for k, (i, name) in enumerate(kern):
    if flts and not any(f in dem[k] for f in flts):
        continue
    end = next(j for j in range(i, len(txt)) if ".end_amdhsa_kernel" in txt[j] or txt[j].startswith("\t.section") and j > i + 5)
    loads = full = part = run = best = 0
    vg = "?"
    for l in txt[end:]:
        m = re.match(r"\s*\.set %s\.num_vgpr, (\d+)" % re.escape(name), l)
        if m:
            vg = m.group(1)
            break
    for l in txt[i:end]:
        s = l.strip()
        if re.match(r"(global|buffer|flat)_load", s):
            loads += 1
            run += 1
            best = max(best, run)
        elif s.startswith("s_waitcnt") and "vmcnt" in s:
            run = 0
            if "vmcnt(0)" in s:
                full += 1
            else:
                part += 1
    print(f"{loads:5d} {full:10d} {part:13d} {best:11d} {vg:>5} {dem[k][:100]}")
