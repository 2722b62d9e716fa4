"""CPU test of the one-definition rule inside libvoge_hip.so, as a text scan (no compiler): every unit of the Makefile's SRCS and
the headers it includes are linked into ONE library, so a namespace-scope type or a kernel may be defined by one file only.  Two
files that define `voge::X` differently are undefined behaviour even while every use is inlined, and two kernels of one short name
are one line in every trace."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voge_amd", "csrc")
INCLUDE_DIRS = (CSRC, os.path.join(ROOT, "include"))


def units(csrc=CSRC):
    mk = open(os.path.join(csrc, "Makefile")).read()
    return re.search(r"^SRCS\s*:?=\s*(.*)$", mk, flags=re.M).group(1).split()


def strip(src):
    """The text without comments, string and character literals."""
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', src)
    return re.sub(r"'(?:\\.|[^'\\\n])+'", "' '", src)


def closure(unit, dirs):
    """The unit's path and those of the project headers it includes, directly or through another header."""
    todo, seen = [os.path.join(dirs[0], unit)], []
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.append(path)
        for inc in re.findall(r'^\s*#\s*include\s*"([^"]+)"', open(path).read(), flags=re.M):
            hits = [os.path.join(d, inc) for d in dirs if os.path.exists(os.path.join(d, inc))]
            todo.extend(hits[:1])
    return seen


TYPE = re.compile(r"\b(?:struct|class|union|enum(?:\s+(?:class|struct))?)\s+(?:(?:alignas|__align__)\s*\([^)]*\)\s*|__attribute__\s*\(\((?:[^()]|\([^()]*\))*\)\)\s*)*(\w+)\s*(?:final\s*)?(?::[^;{()]*)?\{")
SCOPE = re.compile(r'\b(?:namespace(?:\s+\w+)?|extern\s*"")\s*\{')


def definitions(path):
    """(types, kernels): the names of the struct / class / union / named enum definitions at namespace scope and of the __global__
    functions of one file."""
    src = strip(open(path).read())
    bare, at = "", 0
    for m in re.finditer(r"__(?:launch_bounds|attribute)__\s*\(", src):      # (dropped with their balanced argument lists)
        if m.start() < at:
            continue
        bare, at, depth = bare + src[at:m.start()] + " ", m.end(), 1
        while depth:
            depth += {"(": 1, ")": -1}.get(src[at], 0)
            at += 1
    bare += src[at:]
    kernels = set(re.findall(r"\b__global__\s+(?:[\w:]+\s+)*?(\w+)\s*\(", bare))
    types = set()
    depth, at = 0, 0      # depth counts the braces that are not a namespace's or a linkage block's
    transparent = []      # one entry per open brace: does it count?
    while at < len(src):
        if depth == 0:
            s, t = SCOPE.match(src, at), TYPE.match(src, at)
            if s:
                transparent.append(True)
                at = s.end()
                continue
            if t and (at == 0 or not (src[at - 1].isalnum() or src[at - 1] == "_")):
                types.add(t.group(1))
                transparent.append(False)
                depth += 1
                at = t.end()
                continue
        c = src[at]
        if c == "{":
            transparent.append(False)
            depth += 1
        elif c == "}" and transparent:
            depth -= 0 if transparent.pop() else 1
        at += 1
    return types, kernels


def clashes(csrc=CSRC, dirs=INCLUDE_DIRS):
    """{name: the files that define it} for every name that more than one file of the library defines."""
    files = []
    for u in units(csrc):
        files += [p for p in closure(u, dirs) if p not in files]      # (a header counts once: it is one definition)
    where = {}
    for p in files:
        types, kernels = definitions(p)
        for n in types | kernels:
            where.setdefault(n, set()).add(os.path.basename(p))
    return {n: sorted(f) for n, f in where.items() if len(f) > 1}


def test_the_scan_sees_the_library():
    files = {os.path.basename(p) for u in units() for p in closure(u, INCLUDE_DIRS)}
    assert {"knn.hip", "chamfer.hip", "point_mesh.hip", "point_mesh_grid.h", "knn_grid.h", "mesh_scan.h", "voge_common.h", "fixed_point.h"} <= files
    types, kernels = definitions(os.path.join(CSRC, "fixed_point.h"))
    assert "FixedHead" in types and not kernels      # (a kernel in a header is emitted by every unit that includes it)
    types, kernels = definitions(os.path.join(CSRC, "knn_grid.h"))
    assert "KnnGrid" in types and "knn_scan_final_kernel" in kernels
    types, kernels = definitions(os.path.join(CSRC, "knn.hip"))
    assert {"knn_search_kernel", "knn_frames_kernel", "knn_count_kernel"} <= kernels and "KnnLayout" in types
    types, _ = definitions(os.path.join(CSRC, "mesh_sample.hip"))
    assert "MsLayout" in types
    # attributes between __global__ and the name are no names
    _, kernels = definitions(os.path.join(CSRC, "fragment_bwd.hip"))
    assert "fragment_bwd_kernel" in kernels and not [k for k in kernels if k.startswith("__")]


def test_no_name_is_defined_by_two_files():
    found = clashes()
    assert not found, "defined by more than one file of libvoge_hip.so: " + "; ".join(f"{n} ({', '.join(f)})" for n, f in sorted(found.items()))
