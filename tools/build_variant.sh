#!/bin/bash
# Build a variant of libssv_hip.so with extra compiler flags:  tools/build_variant.sh NAME -DSSV_XYZ=1 ...
# -> spoofsv_amd/csrc/build/ab/libssv_hip_NAME.so (git-ignored; travels to the GPU box).  Use with SSV_HIP_LIB=<path>.
# (The csrc Makefile does the work -- its source list and per-file flags are the only ones: make -C spoofsv_amd/csrc VARIANT=NAME EXTRA="...")
set -e
name=$1; shift
exec make -C "$(dirname "$0")/../spoofsv_amd/csrc" -j16 VARIANT="$name" EXTRA="$*"
