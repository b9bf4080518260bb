#!/bin/bash
# Build an experimental variant of libpem_hip.so: tools/build_variant.sh <name> [-DMACRO=1 ...]
# -> build_variants/libpem_<name>.so (git-ignored, but it travels to the GPU box with gpurun)
# The translation units are those of the regular build (hallthrusterpem_amd/build.py SRCS).
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p build_variants
srcs=$(python -c "from hallthrusterpem_amd import build; print(' '.join(str(s.relative_to(build.ROOT)) for s in build.SRCS))")
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Iinclude -Ihallthrusterpem_amd/csrc "$@" \
    $srcs -o build_variants/libpem_$name.so
echo build_variants/libpem_$name.so
