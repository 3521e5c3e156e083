#!/bin/bash
# usage: bash scripts/build_variant.sh <tag> [extra hipcc -D flags...]  ->  opencl_render_amd/variants/lib_<tag>.so
# Same sources and exactness flags as csrc/Makefile; only rt_wavefront.hip (the frame's kernels) is recompiled with the extra defines;
# the scene passes of rt_scene_passes.hip are linked as the Makefile built them.
set -e
tag=$1; shift
cd "$(dirname "$0")/../opencl_render_amd/csrc"
make -s
mkdir -p build ../variants
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -fno-gpu-rdc \
    -I../../include -I. "$@" -c rt_wavefront.hip -o build/wf_$tag.o
# the Makefile's own object list, rt_wavefront.o replaced by the variant (so the two lists cannot drift apart)
objs=$(make -s objs | sed "s#/build/rt_wavefront\.o#/build/wf_$tag.o#")
case "$objs" in *"/build/wf_$tag.o"*) ;; *) echo "build_variant.sh: rt_wavefront.o is not in the Makefile's OBJS" >&2; exit 1 ;; esac
/opt/rocm/bin/hipcc -shared -fPIC -o ../variants/lib_$tag.so $objs -pthread
echo built opencl_render_amd/variants/lib_$tag.so
