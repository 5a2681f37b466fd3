#!/bin/bash
# Diagnostic library: per-row, per-phase s_memtime stamps of the numeric rows and the flight
# recorder (-DMHS_ROW_STAMPS=1; read by tools/diag/stamps2.py and tools/diag/flight.py), built
# into tools/diag/stamps/ (git-ignored; travels to the GPU box).  Extra -D flags: "$@".
set -e
here=$(cd "$(dirname "$0")" && pwd)
OUT=$here $here/../build_variant.sh ${OUT:-stamps} -DMHS_ROW_STAMPS=1 "$@"
