#!/bin/bash
# timing-only build of the library with pconv.hip's phase counters: tune/lib_phases.so (tools/probe_phases.py).  Links the
# -DPC_PHASES object of pconv.hip against the other objects `make` writes in build/.
cd "$(dirname "$0")/.." || exit 1
make -s -j8 >/dev/null || exit 1
mkdir -p scratch/phases tune
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wall -Wno-unused-function -DPC_PHASES -c fedmlp_amd/csrc/pconv.hip -o scratch/phases/pconv_phases.o &&
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tune/lib_phases.so $(ls build/*.o | grep -v '/pconv.o') scratch/phases/pconv_phases.o && echo tune/lib_phases.so
