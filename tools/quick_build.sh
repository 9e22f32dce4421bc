#!/bin/bash
# Experiment build beside the tree: tools/quick_build.sh [N,NS,HC[;N,NS,HC...]] [extra hipcc flags]
# Runs build.py on a copy of the sources with VSMPC_HORIZONS / VSMPC_HIPCC_FLAGS set and writes $Q/libvsmpc.so (or
# $QUICK_OUT/libvsmpc.so); the tracked csrc/vsmpc_horizons.def and the library of the tree are left alone.
set -e
cd "$(dirname "$0")/.."
PKG=paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd
H=${1:-17,7,12}; shift || true
Q=${QUICK_OUT:-exp/quick}
rm -rf $Q/src && mkdir -p $Q/src/$PKG/csrc $Q/src/include
cp $PKG/build.py $Q/src/$PKG/
cp $PKG/csrc/*.hip $PKG/csrc/*.hpp $PKG/csrc/*.inc $Q/src/$PKG/csrc/
cp include/*.h $Q/src/include/
VSMPC_HORIZONS="$H" VSMPC_HIPCC_FLAGS="$*" python3 $Q/src/$PKG/build.py > $Q/build.log 2>&1 || { cat $Q/build.log; exit 1; }
cp $Q/src/$PKG/libvsmpc.so $Q/libvsmpc.so
echo "built $Q/libvsmpc.so for horizon $H"
