#!/bin/bash
# A/B builds of the kernel files: scripts/ab_build.sh NAME "-DFOO=1 ..." -> gnn_computing_amd/csrc/build/ab/libgnnagg_NAME.so
# (select at run time with GNNAGG_LIB=<path>).  The second argument goes to every kernel file's compile line: -mllvm options, or the -D of
# a patched tree.  The shipped sources have no compile-time switch left: to rebuild a retired form, apply scripts/attic/ab_switches_retired.patch
# (or gemm_switches_retired.patch, on the commit it names) to a copy of the tree and run that copy's ab_build.sh with the switch's -D.
set -e
cd "$(dirname "$0")/../gnn_computing_amd/csrc"
make -s -j4
mkdir -p build/ab
objs=""
for f in $(make -s print-kfiles); do   # the Makefile's list of kernel files
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -mllvm -amdgpu-mfma-vgpr-form $2 -c $f.hip -o build/ab/${f}_$1.o &
  objs="$objs build/ab/${f}_$1.o"
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build/ab/libgnnagg_$1.so $objs build/api.o build/api_flat.o build/api_extras.o build/host_graph.o build/reorder.o build/dist_rccl.o -lgomp -ldl -Wl,--exclude-libs,ALL
echo build/ab/libgnnagg_$1.so
