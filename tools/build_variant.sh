#!/bin/bash
# A variant build of the library for same-box A/B runs: tools/build_variant.sh <name> [extra hipcc flags ...]
#   -> cytospace_amd/build/libcytohip_<name>.so (git-ignored, travels to the GPU box); run with CYTOHIP_LIB=$GRAFT_REPO_ROOT/cytospace_amd/build/libcytohip_<name>.so
# e.g.  tools/build_variant.sh coop0 -DCYTO_COOP_MIN_N=0      (tools/run/r06r.sh, r06z.sh)
#       tools/build_variant.sh stop128 -DWIDE_STOP_CAP=128
#       VARIANT_SRCS=lap_jv.hip tools/build_variant.sh probe1 -DCYTO_COLRED_PROBE=1
# Only the sources in VARIANT_SRCS (default: the wide solver's three, lap_wide.hip lap_wide_rr.hip lap_wide_drv.hip) are recompiled with the flags; the other objects come from the last
# `python -m cytospace_amd.build` (VARIANT_NO_BASE=1: do not run it again first -- several variants built side by side).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
srcs=${VARIANT_SRCS:-lap_wide.hip lap_wide_rr.hip lap_wide_drv.hip}
[ -n "$VARIANT_NO_BASE" ] || python -m cytospace_amd.build > /dev/null
vobjs=""
for s in $srcs; do
  o=$R/cytospace_amd/build/${s%.hip}_$name.o
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result "$@" -c -o $o $R/cytospace_amd/csrc/$s
  vobjs="$vobjs $o"
done
# (the other objects: build.SOURCES, so that a new source file cannot be forgotten here)
objs=$(cd $R && VSRCS="$srcs" python -c "import os; from cytospace_amd import build as b; v = os.environ['VSRCS'].split(); print(' '.join(os.path.join(b.OBJ, s.replace('.hip', '.o')) for s in b.SOURCES if s not in v))")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/cytospace_amd/build/libcytohip_$name.so $objs $vobjs -L/opt/rocm/lib -lrccl -lpthread
ls -la $R/cytospace_amd/build/libcytohip_$name.so
