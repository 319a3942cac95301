#!/usr/bin/env python3
"""oracle/build_reference_torch_ext.py -- the drop-in claim at the PyTorch boundary, exercised: the REFERENCE's own torch
binding (/root/reference/Figure7/kernel.cpp: pybind wrappers over ten flat functions + new_load), translated where it lies by
ROCm's hipify-perl (no hand edits) into a scratch directory whose ../include is THIS repo's include/compat, compiled with
torch.utils.cpp_extension together with drivers/flat_cxx_linkage.cpp and linked with libgnnagg.so.  Output:
oracle/_ref/drivers/gnncompile.so (git-ignored; tests/test_gpu_reference.py imports it and runs the reference's Python-level call
sequence, Figure7/our.py:171-188).  Skips quietly when the reference tree or hipify-perl is missing."""
import glob
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("REF", "/root/reference")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
OUT = os.path.join(HERE, "_ref", "drivers", "gnncompile.so")
STAMP = OUT + ".inputs"   # sha-256 of every input, this recipe included, of the build that wrote OUT
LINKAGE = os.path.join(ROOT, "drivers", "flat_cxx_linkage.cpp")


def inputs_digest():
    deps = [os.path.join(REF, "Figure7", "kernel.cpp"), LINKAGE, os.path.abspath(__file__),
            os.path.join(ROOT, "include", "gnnagg.h")] + sorted(glob.glob(os.path.join(ROOT, "include", "compat", "*.h")))
    h = hashlib.sha256()
    for d in deps:
        h.update(open(d, "rb").read())
    return h.hexdigest()


def up_to_date():
    """By content, not by time stamps: a gnncompile.so copied in from another build (newer than a fresh checkout's files) is rebuilt
    unless it was made by this very recipe from these very inputs."""
    if not os.path.exists(OUT) or not os.path.exists(STAMP) or os.environ.get("FORCE"):
        return False
    return open(STAMP).read().strip() == inputs_digest()


def main():
    hipify = os.path.join(ROCM, "bin", "hipify-perl")
    src = os.path.join(REF, "Figure7", "kernel.cpp")
    if not os.path.exists(src) or not os.path.exists(hipify):
        print("oracle/_ref/drivers/gnncompile.so: no reference tree: not built")
        return
    if up_to_date():
        print("oracle/_ref/drivers/gnncompile.so is up to date")
        return
    from torch.utils.cpp_extension import load
    gen = tempfile.mkdtemp(prefix="gnnreftorch.")
    try:
        os.makedirs(os.path.join(gen, "Figure7"))
        os.symlink(os.path.join(ROOT, "include", "compat"), os.path.join(gen, "include"))   # kernel.cpp includes "../include/util.h"
        with open(os.path.join(gen, "Figure7", "kernel.cpp"), "w") as f:
            subprocess.check_call([hipify, src], stdout=f, stderr=subprocess.DEVNULL)
        # libgnnagg.so is found first relative to the installed gnncompile.so ($ORIGIN = oracle/_ref/drivers): the built file travels with
        # a copy of the tree, where the absolute path of this tree does not exist.  The absolute path after it serves load()'s own import
        # of the library in the scratch directory.  ($$ is ninja's escape of `$`, \ the shell's.)
        load(name="gnncompile", sources=[os.path.join(gen, "Figure7", "kernel.cpp"), LINKAGE],
             extra_include_paths=[os.path.join(ROCM, "include"), os.path.join(ROCM, "include", "hiprand"), os.path.join(ROCM, "include", "hipblas"),
                                  os.path.join(ROOT, "include")],
             extra_cflags=["-D__HIP_PLATFORM_AMD__", "-w", "-std=c++17"],
             extra_ldflags=["-L" + os.path.join(ROOT, "gnn_computing_amd"), "-lgnnagg", "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-lhiprand",
                            "-lhipblas", r"-Wl,-rpath,\$$ORIGIN/../../../gnn_computing_amd",
                            "-Wl,-rpath," + os.path.join(ROOT, "gnn_computing_amd"), "-Wl,-rpath," + os.path.join(ROCM, "lib")],
             build_directory=gen, verbose=False, is_python_module=False)
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        shutil.copy(os.path.join(gen, "gnncompile.so"), OUT)
        with open(STAMP, "w") as f:
            f.write(inputs_digest() + "\n")
        print("oracle/_ref/drivers/gnncompile.so: the reference's Figure7/kernel.cpp built against include/compat + libgnnagg.so")
    finally:
        shutil.rmtree(gen, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
