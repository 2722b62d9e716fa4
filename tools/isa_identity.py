#!/usr/bin/env python
"""Are the hot kernels' machine code bodies the same at two commits?  (No GPU needed: hipcc emits gfx950 assembly.)

usage: tools/isa_identity.py [parent-commit, default HEAD]      (head = the working tree)

Compiles fragment_bwd.hip and composite.hip of both trees with the product flags to assembly, cuts out the instantiations
named below (the five of tests/test_isa_cpu.py and the wave-form composite + shade the cfg3 frame launches), replaces the
function-numbered labels `.LBB<n>_<m>` by `.LBB_<m>` -- a new instantiation in front renumbers them -- and compares the bodies
line by line.  Prints one line per kernel with both register counts; exit status 1 if any body differs (the first differing
lines are shown)."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = {
    "fragment_bwd": ["fragment_bwd_kernelILi0ELi3ELi2EjLb1ELb1ELb0E", "fragment_bwd_kernelILi0ELi4ELi2EjLb1ELb1ELb0E",
                     "fragment_bwd_kernelILi1ELi0ELi2EjLb1ELb1ELb0E", "fragment_bwd_kernelILi0ELi3ELi2EjLb0ELb1ELb1E",
                     "fragment_bwd_kernelILi0ELi3ELi2EjLb0ELb0ELb0E"],
    "composite": ["compositen_kernelILi0ELi4ELb1EjLi3ELi0E"],      # <MODE 0, NS 4, WAVE, u32 offsets, SC 3, GEN 0>
}


def asm(tree, unit, out):
    csrc = os.path.join(tree, "voge_amd", "csrc")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                           "-I" + os.path.join(tree, "include"), "-I" + csrc, "-S", "--offload-device-only", "-o", out,
                           os.path.join(csrc, unit + ".hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


def kernel(text, fragment):
    m = re.search(r"^(_ZN4voge\w*" + re.escape(fragment) + r"\w*):\s", text, flags=re.M)
    assert m, fragment
    body = text[m.start():text.index(".Lfunc_end", m.start())]
    d = text.index(".amdhsa_kernel " + m.group(1))
    desc = text[d:text.index(".end_amdhsa_kernel", d)]
    regs = tuple(int(re.search(r"\." + k + r"\s+(\d+)", desc).group(1)) for k in ("amdhsa_next_free_vgpr", "amdhsa_next_free_sgpr"))
    body = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", body)
    lines = [l.split(";", 1)[0].rstrip() for l in body.splitlines()]      # (comments carry no code, but they do carry block numbers)
    return [l for l in lines if l], regs


def main():
    parent = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        ptree = os.path.join(tmp, "parent")
        os.makedirs(ptree)
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", parent, "voge_amd/csrc", "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", ptree], stdin=tar.stdout)
        assert tar.wait() == 0
        for unit, frags in KERNELS.items():
            a, b = asm(ptree, unit, os.path.join(tmp, unit + "_parent.s")), asm(ROOT, unit, os.path.join(tmp, unit + "_head.s"))
            for frag in frags:
                (pb, pr), (hb, hr) = kernel(a, frag), kernel(b, frag)
                same = pb == hb
                differ += not same
                print(f"{frag:48s} {'IDENTICAL' if same else 'DIFFERS  '} {len(hb):6d} lines   vgpr/sgpr parent {pr[0]}/{pr[1]}  head {hr[0]}/{hr[1]}")
                if not same:
                    for line in list(difflib.unified_diff(pb, hb, "parent", "head", lineterm="", n=1))[:40]:
                        print("    " + line)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
