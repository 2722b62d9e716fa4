"""Build the reference's own native extension for gfx950 into oracle/_ref/ -- TEST INFRASTRUCTURE.

The reference ships CUDA sources only (VoGE/csrc: ext.cpp + four .cu units).  The installed ROCm torch
hipifies such sources inside ``torch.utils.cpp_extension.load``, so they cross-compile for gfx950 once

  * ``-DWITH_CUDA`` is on the host and the device command line (the reference's setup.py defines it; without it
    the headers expand to AT_ERROR(...) at file scope), and
  * the float ``atomicMax`` helper of sample_voge.cu is renamed in the copy: HIP declares
    ``atomicMax(float*, float)`` itself, non-static, and the file's ``static`` one clashes with it.

Nothing of the reference is kept: the sources are copied into a build directory under oracle/_ref/ (the hipifier
writes beside its inputs and the reference tree is read-only), built, and the copy, the hipified files and the
ninja directory are deleted again.  What stays is oracle/_ref/voge_ref_C.so and oracle/_ref/BUILD_INFO.json;
oracle/_ref/ is git-ignored.  tests/ref_kernels.py loads the .so by path.
"""
import json
import os
import re
import shutil
import sys
import time

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
SO_PATH = os.path.join(REF_DIR, "voge_ref_C.so")
INFO_PATH = os.path.join(REF_DIR, "BUILD_INFO.json")
MODULE_NAME = "voge_ref_C"
DEFAULT_REFERENCE = "/root/reference"        # the default tests/golden/make_golden.py uses
ARCH = "gfx950"
FLAGS = ["-DWITH_CUDA", "-O2"]
RENAMED = {"file": "sample_voge/sample_voge.cu", "from": "atomicMax", "to": "vogeRefAtomicMaxF"}
SOURCES = ["ext.cpp", "rasterize_coarse/rasterize_coarse.cu", "ray_trace_voge/ray_trace_voge.cu",
           "sample_voge/sample_voge.cu", "voge_ray_tracing_ray/voge_ray_tracing_ray.cu"]
NAMES = ("rasterize_points_coarse", "ray_trace_voge_fine", "ray_trace_voge_fine_backward", "ray_trace_voge_ray",
         "ray_trace_voge_ray_backward", "find_nearest_k", "sample_voge", "sample_voge_backward", "scatter_max")


def reference_dir():
    return os.environ.get("VOGE_REFERENCE", DEFAULT_REFERENCE)


def reference_csrc():
    return os.path.join(reference_dir(), "VoGE", "csrc")


def have_reference():
    return os.path.isfile(os.path.join(reference_csrc(), "ext.cpp"))


def build(force=False, verbose=False):
    """Returns the path of the .so, or None where neither the reference nor an earlier .so exists."""
    if not have_reference():
        kept = os.path.exists(SO_PATH)
        print(f"oracle/_ref: no reference sources at {reference_csrc()}; nothing built, "
              + ("keeping the existing voge_ref_C.so" if kept else "no voge_ref_C.so present"))
        return SO_PATH if kept else None
    if not force and os.path.exists(SO_PATH) and os.path.exists(INFO_PATH):
        return SO_PATH

    import torch
    from torch.utils import cpp_extension

    os.makedirs(REF_DIR, exist_ok=True)
    work = os.path.join(REF_DIR, "_build")
    shutil.rmtree(work, ignore_errors=True)
    src = os.path.join(work, "csrc")
    ninja_dir = os.path.join(work, "ninja")
    shutil.copytree(reference_csrc(), src)
    os.makedirs(ninja_dir)
    os.chmod(src, 0o755)
    for root, dirs, files in os.walk(src):          # the reference tree is read-only; the copy must not be
        for n in dirs + files:
            os.chmod(os.path.join(root, n), 0o755 if n in dirs else 0o644)

    path = os.path.join(src, RENAMED["file"])
    with open(path) as f:
        text = f.read()
    text, n = re.subn(r"\b%s\b" % RENAMED["from"], RENAMED["to"], text)
    assert n > 0, "the identifier to rename was not found"
    with open(path, "w") as f:
        f.write(text)

    saved = {k: os.environ.get(k) for k in ("PYTORCH_ROCM_ARCH", "MAX_JOBS")}
    os.environ["PYTORCH_ROCM_ARCH"] = ARCH
    jobs = min(16, int(saved["MAX_JOBS"] or 8))
    os.environ["MAX_JOBS"] = str(jobs)
    t0 = time.time()
    try:
        cpp_extension.load(name=MODULE_NAME, sources=[os.path.join(src, s) for s in SOURCES],
                           extra_include_paths=[src], extra_cflags=FLAGS, extra_cuda_cflags=FLAGS,
                           build_directory=ninja_dir, with_cuda=True, is_python_module=True, verbose=verbose)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    seconds = time.time() - t0
    shutil.copyfile(os.path.join(ninja_dir, MODULE_NAME + ".so"), SO_PATH)
    shutil.rmtree(work)
    sys.modules.pop(MODULE_NAME, None)              # tests/ref_kernels.py loads the kept file by path
    with open(INFO_PATH, "w") as f:
        json.dump({"torch": torch.__version__, "hip": torch.version.hip, "arch": ARCH, "flags": FLAGS,
                   "max_jobs": jobs,
                   "renamed": RENAMED, "sources": SOURCES, "build_seconds": round(seconds, 1)}, f, indent=1)
        f.write("\n")
    print(f"oracle/_ref: built voge_ref_C.so for {ARCH} in {seconds:.0f} s")
    return SO_PATH


if __name__ == "__main__":
    build(force=True, verbose="-v" in sys.argv)
