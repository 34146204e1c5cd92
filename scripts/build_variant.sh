#!/bin/bash
# Build one experiment variant of libpob.so into build_variants/NAME.so:
#   bash scripts/build_variant.sh NAME -DPOB_EXP_...
set -e
NAME=$1; shift
cd "$(dirname "$0")/.."
mkdir -p build_variants
# the sources and the flags are the build's own (__graft_entry__.py)
SRCS=$(python3 -c "import os, __graft_entry__ as g; print(*[os.path.join(g.CSRC, f) for f in g.HIP_SOURCES])")
FLAGS=$(python3 -c "import __graft_entry__ as g; print(*g.HIPCC_FLAGS)")
/opt/rocm/bin/hipcc $FLAGS -shared "$@" -o build_variants/.$NAME.tmp $SRCS
mv build_variants/.$NAME.tmp build_variants/$NAME.so  # (atomic: a GPU snapshot never sees half a library)
