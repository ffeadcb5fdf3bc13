#!/bin/bash
# Tuning build of the working tree's production libpdd with extra defines
# (PDD_FX_GT, PDD_FX_PAIR_MAX, ...) into build/libpdd_<name>.so, loaded with
# PDD_DEV_LIB=build/libpdd_<name>.so:  scripts/build_variant.sh <name> [-DFOO=1 ...]
# (developer knobs -- stamps, timing-only decompositions: scripts/build_dev.sh)
# Sources and flags: pypulsar_amd/_digest.py, the production build's own list.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p build
SRCS=$(python3 -c "from pypulsar_amd import _digest as d; print(' '.join('pypulsar_amd/csrc/' + s for s in d.SOURCES))")
FLAGS=$(python3 -c "from pypulsar_amd import _digest as d; print(' '.join(d.FLAGS))")
/opt/rocm/bin/hipcc $FLAGS "$@" -o build/libpdd_$name.so $SRCS
