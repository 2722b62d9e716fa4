#!/usr/bin/env python3
"""Static instruction counts of one kernel, itemised by the source lines they came from (no GPU needed).

usage: tools/isa_sections.py unit mangled-fragment [file:lo-hi=name ...] [-DFLAG ...]      (unit: a name in voge_amd/csrc or a path to a .hip)

Compiles voge_amd/csrc/<unit>.hip for gfx950 with the flags of tools/asm.sh plus -gline-tables-only (line tables only: the
instructions are those of the product build, which the total printed first lets one check), follows the .loc directives of
the one kernel whose mangled name contains the fragment, and prints VALU / SALU / LDS / VMEM counts per named range of source
lines (innermost inlined location; first matching range wins; everything else under "other") and the commonest VALU opcodes."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voge_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def kind(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op.startswith("s_cbranch") or op.startswith("s_branch"):
        return "branch"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_endpgm")):
        return "wait"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "SMEM"
    return "SALU" if op.startswith("s_") else "?"


def main(argv):
    unit, frag = argv[0], argv[1]
    ranges = []
    flags = []
    for a in argv[2:]:
        m = re.match(r"([\w.]+):(\d+)-(\d+)=(.+)", a)
        if m:
            ranges.append((m.group(1), int(m.group(2)), int(m.group(3)), m.group(4)))
        else:
            flags.append(a)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                               "-gline-tables-only", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--offload-device-only"]
                              + flags + ["-o", out, unit if unit.endswith(".hip") else os.path.join(CSRC, unit + ".hip")], stderr=subprocess.DEVNULL)
        text = open(out).read()
    files = {int(n): os.path.basename(f) for n, f in re.findall(r'^\s*\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]+)"', text, flags=re.M)}
    m = re.search(r"^(_ZN4voge\w*" + re.escape(frag) + r"\w*):\s", text, flags=re.M)
    assert m, frag
    body = text[m.start():text.index(".Lfunc_end", m.start())]
    per = collections.defaultdict(collections.Counter)
    ops = collections.Counter()
    lines = collections.Counter()
    where = ("?", 0)
    for raw in body.splitlines():
        line = raw.strip()
        l = re.match(r"\.loc\s+(\d+)\s+(\d+)", line)
        if l:
            where = (files.get(int(l.group(1)), "?"), int(l.group(2)))
            continue
        if not line or line.startswith((";", ".", "_Z")) or line.endswith(":"):
            continue
        op = line.split()[0]
        name = "other"
        for f, lo, hi, n in ranges:
            if where[0] == f and lo <= where[1] <= hi:
                name = n
                break
        per[name][kind(op)] += 1
        if kind(op) == "VALU":
            ops[re.sub(r"_e(32|64)$|_dpp$|_sdwa$", "", op)] += 1
            if name == "other":
                lines[where] += 1
    cols = ("VALU", "SALU", "LDS", "VMEM", "SMEM", "branch", "wait")
    print(m.group(1))
    print("%-28s" % "section" + "".join("%8s" % c for c in cols))
    order = [n for _, _, _, n in ranges]
    for name in list(dict.fromkeys(order)) + ["other"]:
        if name in per:
            print("%-28s" % name + "".join("%8d" % per[name][c] for c in cols))
    print("%-28s" % "total" + "".join("%8d" % sum(p[c] for p in per.values()) for c in cols))
    print("VALU opcodes:", ", ".join("%s %d" % kv for kv in ops.most_common(14)))
    if lines:
        print("unnamed lines with most VALU:", ", ".join("%s:%d %d" % (f, n, c) for (f, n), c in lines.most_common(12)))


if __name__ == "__main__":
    main(sys.argv[1:])
