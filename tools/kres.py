"""Kernel resources from hipcc -Rpass-analysis=kernel-resource-usage output: python3 tools/kres.py A.txt [B.txt]
(prints every sqp_step_kernel instantiation's registers, spills, scratch, occupancy and LDS; with two files,
every instantiation with what differs, "same" where nothing does)."""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
          "VGPRs Spill", "LDS Size [bytes/block]")


def parse(f):
    out, cur = {}, None
    for line in open(f):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"\s(" + "|".join(re.escape(k) for k in FIELDS) + r"): (\d+)", line)
        if m and cur:
            out[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return out


a = parse(sys.argv[1])
b = parse(sys.argv[2]) if len(sys.argv) > 2 else None
for k in a:
    if "sqp_step" not in k:
        continue
    n = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
    n = n.replace("void gpmpc::sqp_step_kernel", "").split("(")[0]
    if b is None:
        print(n, a[k])
    else:
        diff = {f: (b.get(k, {}).get(f), v) for f, v in a[k].items() if b.get(k, {}).get(f) != v}
        print(n, "same as B" if not diff else f"(B, A) {diff}", "|", a[k])
