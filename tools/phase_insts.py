#!/usr/bin/env python3
"""Static instruction mix per clip phase of the FAST extraction kernel (diagnostic).

Compiles extract.hip with -DDSP_MARKS (region labels ``;@@ NAME`` from MARK() in clip_fast) to
gfx950 assembly and counts, in layout order from each label to the next, the VALU / SALU / LDS /
vector-memory instructions, the wait states the compiler inserted (the no-op mnemonic ``s_nop``, a
column of its own beside the other control instructions) and the backward branches (loops, whose
bodies run more than once).
Static counts: straight-line regions (R1, R2) are exact per wave; loop regions (pass A/B, R4)
are per iteration.

    python tools/phase_insts.py [extra hipcc -D flags...]
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "dsp-audioreclabs_amd", "csrc")
KERNEL = "_ZN3dsp14extract_kernelILb1EEEvNS_13ExtractParamsE"


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op == "s_nop":
        return "s_nop"
    if op in ("s_waitcnt", "s_barrier", "s_setprio", "s_sleep") or op.startswith("s_cbranch") or \
            op == "s_branch":
        return "ctl"
    if op.startswith("s_"):
        return "salu"
    return None


def main():
    out = os.path.join(tempfile.mkdtemp(), "k.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I../../include",
                    "-Wno-unused-function", "-mllvm", "-amdgpu-use-amdgpu-trackers=1", "--offload-device-only", "-S", "extract.hip", "-o", out, "-DDSP_MARKS"]
                   + sys.argv[1:], cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
    s = open(out).read()
    a = s.index(KERNEL + ":")
    body = s[a:s.index(".Lfunc_end", a)].split("\n")
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
    region, cnt = "prologue", collections.defaultdict(collections.Counter)
    for i, l in enumerate(body):
        t = l.strip()
        m = re.match(r"^;@@ (\w+)", t)
        if m:
            region = m.group(1)
            continue
        if not t or t.startswith((";", ".")) or t.endswith(":"):
            continue
        op = t.split()[0]
        k = classify(op)
        if k:
            cnt[region][k] += 1
        if op.startswith("s_cbranch") or op == "s_branch":
            tgt = t.split()[-1]
            if labels.get(tgt, 1 << 30) < i:
                cnt[region]["back_branches"] += 1
    keys = ("valu", "salu", "lds", "vmem", "ctl", "s_nop", "back_branches")
    print("%-10s" % "region" + "".join("%8s" % k[:8] for k in keys))
    tot = collections.Counter()
    for r, c in cnt.items():
        print("%-10s" % r + "".join("%8d" % c[k] for k in keys))
        tot.update(c)
    print("%-10s" % "total" + "".join("%8d" % tot[k] for k in keys))


if __name__ == "__main__":
    main()
