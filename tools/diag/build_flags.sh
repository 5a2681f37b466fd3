#!/bin/bash
# Build flag variants of libmhspgemm into tools/diag/<name>/:
#   tools/diag/build_flags.sh name "-DFOO=1 -DBAR=2" [name2 "flags2" ...]
# (each through the Makefile, as tools/build_variant.sh does)
set -e
here=$(cd "$(dirname "$0")" && pwd)
while [ $# -ge 2 ]; do
  OUT=$here $here/../build_variant.sh "$1" $2
  shift 2
done
