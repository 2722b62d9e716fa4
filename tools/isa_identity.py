#!/usr/bin/env python
"""Is every kernel's machine code body the same at two commits?  (No GPU needed: hipcc emits gfx950 assembly.)

usage: tools/isa_identity.py [-v] [--flags=-DX,-DY] [parent-commit, default HEAD] [old=new ...]      (head = the working tree)

Compiles every unit of voge_amd/csrc/Makefile's SRCS, of both trees, with the product flags to assembly, cuts out every function
whose label starts with `_ZN4voge`, replaces the function-numbered labels `.LBB<n>_<m>` by `.LBB_<m>` -- a new instantiation in
front renumbers them -- and compares the bodies line by line, matched by symbol name.  `old=new` (substrings of the mangled
names) pairs a kernel that was renamed: its own symbol is normalised inside the body too.  `--flags=` appends compile flags
(comma-separated) to both sides: `--flags=-DVOGE_AB` compares the A/B library's units.

Prints one line per unit (`N kernels, all IDENTICAL`; -v: one line per kernel), always the register counts of the six named
kernels below (the five of tests/test_isa_cpu.py and the wave-form composite + shade the cfg3 frame launches), every differing
kernel with its first differing lines and both register counts, and the kernels that exist on one side only.  Exit status 1
on any difference and on any kernel without a partner."""
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXTRA = []      # --flags=
NAMED = ["fragment_bwd_kernelILi0ELi3ELi2EjLb1ELb1ELb0E", "fragment_bwd_kernelILi0ELi4ELi2EjLb1ELb1ELb0E",
         "fragment_bwd_kernelILi1ELi0ELi2EjLb1ELb1ELb0E", "fragment_bwd_kernelILi0ELi3ELi2EjLb0ELb1ELb1E",
         "fragment_bwd_kernelILi0ELi3ELi2EjLb0ELb0ELb0E",
         "compositen_kernelILi0ELi4ELb1EjLi3ELi0E"]      # <MODE 0, NS 4, WAVE, u32 offsets, SC 3, GEN 0>


def units(tree):
    mk = open(os.path.join(tree, "voge_amd", "csrc", "Makefile")).read()
    return [s[:-len(".hip")] for s in re.search(r"^SRCS\s*:?=\s*(.*)$", mk, flags=re.M).group(1).split()]


def asm(tree, unit, out):
    csrc = os.path.join(tree, "voge_amd", "csrc")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                           "-I" + os.path.join(tree, "include"), "-I" + csrc] + EXTRA + ["-S", "--offload-device-only", "-o", out,
                           os.path.join(csrc, unit + ".hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


def kernels(text):
    """{symbol: (body lines, (vgpr, sgpr) | None)} of every voge:: function in a unit's assembly."""
    found = {}
    for m in re.finditer(r"^(_ZN4voge\w+):\s", text, flags=re.M):
        name = m.group(1)
        end = text.find(".Lfunc_end", m.start())
        if end < 0:      # (a constant table behind the last function: data, no code)
            continue
        body = text[m.start():end]
        regs = None
        d = text.find(".amdhsa_kernel " + name + "\n")
        if d >= 0:      # (a device function that was not inlined has no descriptor)
            desc = text[d:text.index(".end_amdhsa_kernel", d)]
            regs = tuple(int(re.search(r"\." + k + r"\s+(\d+)", desc).group(1)) for k in ("amdhsa_next_free_vgpr", "amdhsa_next_free_sgpr"))
        body = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", body)
        lines = [l.split(";", 1)[0].rstrip() for l in body.splitlines()]      # (comments carry no code, but they do carry block numbers)
        found[name] = ([l for l in lines if l], regs)
    return found


def compare(unit, par, head, renames, verbose):
    """Prints the unit's report; returns the number of differing or unmatched kernels."""
    pairs = [(n, n) for n in par if n in head]
    only_p, only_h = [n for n in par if n not in head], [n for n in head if n not in par]
    for old, new in renames:
        po, hn = [n for n in only_p if old in n], [n for n in only_h if new in n]
        if len(po) == 1 and len(hn) == 1:
            pairs.append((po[0], hn[0]))
            only_p.remove(po[0])
            only_h.remove(hn[0])
    bad = 0
    for pn, hn in pairs:
        (pb, pr), (hb, hr) = par[pn], head[hn]
        if pn != hn:
            # (own symbol, and where the linker puts it: a template's instantiation sits in a comdat section of its own name)
            pb, hb = ([l.replace(n, "<self>") for l in b if not re.match(r"\s*\.(section\s+\.text\.<self>|text$)", l.replace(n, "<self>"))]
                      for n, b in ((pn, pb), (hn, hb)))
        same = pb == hb
        bad += not same
        if verbose or not same or pn != hn or any(f in hn for f in NAMED):
            short = hn[len("_ZN4voge"):]
            regs = f"vgpr/sgpr parent {pr[0]}/{pr[1]}  head {hr[0]}/{hr[1]}" if pr and hr else ""
            print(f"  {short:56s} {'IDENTICAL' if same else 'DIFFERS  '} {len(hb):6d} lines   {regs}" + (f"   (was {pn[len('_ZN4voge'):]})" if pn != hn else ""))
        if not same:
            for line in list(difflib.unified_diff(pb, hb, "parent", "head", lineterm="", n=1))[:40]:
                print("      " + line)
    for n in only_p:
        print(f"  {n[len('_ZN4voge'):]}: in the parent only")
    for n in only_h:
        print(f"  {n[len('_ZN4voge'):]}: in the working tree only")
    bad += len(only_p) + len(only_h)
    print(f"{unit}: {len(pairs)} kernels, " + ("all IDENTICAL" if not bad else f"{bad} DIFFER or have no partner"))
    return bad


def main():
    args = [a for a in sys.argv[1:] if a != "-v" and not a.startswith("--flags=")]
    verbose = "-v" in sys.argv[1:]
    EXTRA.extend(f for a in sys.argv[1:] if a.startswith("--flags=") for f in a[len("--flags="):].split(",") if f)
    renames = [tuple(a.split("=", 1)) for a in args if "=" in a]
    commits = [a for a in args if "=" not in a]
    parent = commits[0] if commits else "HEAD"
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        ptree = os.path.join(tmp, "parent")
        os.makedirs(ptree)
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", parent, "voge_amd/csrc", "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", ptree], stdin=tar.stdout)
        assert tar.wait() == 0
        pu, hu = units(ptree), units(ROOT)
        jobs = [(t, tree, u) for t, tree, us in (("parent", ptree, pu), ("head", ROOT, hu)) for u in us]
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            texts = dict(zip([(t, u) for t, _, u in jobs],
                             pool.map(lambda j: asm(j[1], j[2], os.path.join(tmp, j[2] + "_" + j[0] + ".s")), jobs)))
        for u in pu + [u for u in hu if u not in pu]:
            if u not in pu or u not in hu:
                print(f"{u}: in the {'parent' if u in pu else 'working tree'} only")
                bad += 1
                continue
            bad += compare(u, kernels(texts[("parent", u)]), kernels(texts[("head", u)]), renames, verbose)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
