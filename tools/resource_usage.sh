#!/bin/bash
# Per-kernel VGPRs / SGPRs / spills / scratch / occupancy / static LDS of one kernel source (compiler remarks).
# usage: tools/resource_usage.sh [source.hip] [extra hipcc flags]
# source: a file of mh-spgemm_amd/csrc by name, or a path; default mhs_kernels.hip
ROOT=$(cd "$(dirname "$0")/.." && pwd)
src=mhs_kernels.hip
case "$1" in *.hip|*.cpp) src=$1; shift ;; esac
case "$src" in */*) ;; *) src=$ROOT/mh-spgemm_amd/csrc/$src ;; esac
obj=$(mktemp /tmp/mhs_ru.XXXXXX)
trap 'rm -f $obj' EXIT
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$ROOT/include "$@" -x hip -c $src \
    -o $obj -Rpass-analysis=kernel-resource-usage 2>&1 | python3 -c "
import sys, re
rows = []; cur = None
for l in sys.stdin:
    m = re.search(r'remark: Function Name: (\S+)', l)
    if m: cur = {'name': m.group(1)}; rows.append(cur); continue
    m = re.search(r'remark:\s+([\w \[\]/]+?): (\S+) \[', l)
    if m and cur is not None: cur[m.group(1).strip()] = m.group(2)
import subprocess
for r in rows:
    n = subprocess.run(['c++filt', r['name']], capture_output=True, text=True).stdout.strip()
    n = n.replace('mhs::', '').replace('(anonymous namespace)::', '').split('(')[0]
    print(f\"{n:60s} vgpr {r.get('VGPRs','?'):>4} sgpr {r.get('TotalSGPRs','?'):>4} vspill {r.get('VGPRs Spill','?'):>3} sspill {r.get('SGPRs Spill','?'):>4} scratch {r.get('ScratchSize [bytes/lane]','?'):>4} occ {r.get('Occupancy [waves/SIMD]','?'):>2} lds {r.get('LDS Size [bytes/block]','?'):>5}\")
"
