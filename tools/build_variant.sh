#!/bin/bash
# Build a variant libmhspgemm.so with extra -D flags into tools/var/<name>/ (A/B timing
# via MHS_LIB=tools/var/<name>/libmhspgemm.so).  usage: tools/build_variant.sh <name> -DX=.. ...
# The whole library is built through the Makefile, with the variant's flags, into the variant's
# own object directory (tools/var/<name>/obj).
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
out=${OUT:-$ROOT/tools/var}/$name
make -s -j${JOBS:-8} -C $ROOT/mh-spgemm_amd EXTRA="$*" OBJDIR=$out/obj LIB=$out/libmhspgemm.so lib
echo built $out
