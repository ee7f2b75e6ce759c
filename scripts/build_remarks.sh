#!/bin/bash
# Compile-only build of the product with -Rpass-analysis=kernel-resource-usage; prints one line per kernel
# (VGPRs / AGPRs / SGPRs / scratch / occupancy / LDS).  Usage: scripts/build_remarks.sh [out.so] [extra hipcc flags...]
cd "$(dirname "$0")/../unityraytracer_amd" || exit 1
OUT=${1:-/tmp/urt_remarks.so}; shift
# The flags and the source list are build.py's own.  KERNELS_ONLY=1: compile the trace translation units alone (-c each: kernels.hip and
# kernels_basic / _serve / _pool.hip): the trace kernels' numbers in half a minute
FLAGS=$(python3 -c "from build import HIPCC_FLAGS as F; print(' '.join(f for f in F if f != '-shared'))")
SRCS=$(python3 -c "from build import SOURCES as S; print(' '.join('csrc/' + s for s in S))")
if [ -n "$KERNELS_ONLY" ]; then
  : > /tmp/urt_remarks.log
  for src in csrc/kernels.hip csrc/kernels_basic.hip csrc/kernels_serve.hip csrc/kernels_pool.hip; do
    hipcc $FLAGS -Rpass-analysis=kernel-resource-usage "$@" -c $src -o "$OUT" 2>> /tmp/urt_remarks.log || break
  done
else
  hipcc $FLAGS -shared -Rpass-analysis=kernel-resource-usage "$@" -o "$OUT" $SRCS 2> /tmp/urt_remarks.log
fi
rc=$?
grep -E "error" -A6 /tmp/urt_remarks.log | head -40
python3 - <<'PY'
import re, subprocess
rows, cur = [], None
for line in open('/tmp/urt_remarks.log'):
    m = re.search(r'remark: (?:\s*)(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|VGPRs Spill|SGPRs Spill): (.*?) \[-Rpass', line)
    if not m: continue
    k, v = m.group(1), m.group(2)
    if k == 'Function Name':
        cur = {'name': v}; rows.append(cur)
    elif cur is not None:
        cur[k] = v
for r in rows:
    name = subprocess.run(['c++filt', r['name']], capture_output=True, text=True).stdout.strip()
    if 'rocprim' in name: continue                       # library sort / scan kernels of the GPU BVH build
    name = re.sub(r'^(void )?\(anonymous namespace\)::', '', name).split('(')[0]
    print(f"{name:45s} VGPR {r.get('VGPRs','?'):>4} AGPR {r.get('AGPRs','?'):>3} SGPR {r.get('TotalSGPRs','?'):>4} scratch {r.get('ScratchSize [bytes/lane]','?'):>4} B/lane  "
          f"spill v{r.get('VGPRs Spill','?')} s{r.get('SGPRs Spill','?')}  occupancy {r.get('Occupancy [waves/SIMD]','?')}  LDS {r.get('LDS Size [bytes/block]','?')}")
PY
exit $rc
