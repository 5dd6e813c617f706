#!/bin/bash
# Same-box A/B builds (dev aid; nothing here ships).
#   tools/ab_build.sh rev <revA> [revB=working tree] -> gym_pomdp_amd/_lib/libpomdp_hip_a.so / _b.so from two git revisions
#       (revisions from round 3 on: the library is built by gym_pomdp_amd/_native.py, one object per translation unit);
#       tools/gpu_small_shards.py and tools/gpu_ab_bench.py take such variants by path.  To A/B a gate, change its constant
#       in kernels_common.hip.h in a worktree and build both revisions.
set -e
mode=$1; shift
build() {  # <source tree> <output .so>
  (cd $1 && python - "$2" <<'PY'
import sys
sys.path.insert(0, ".")
from gym_pomdp_amd import _native
print(_native.build(force=True, out=sys.argv[1]))
PY
  )
}
if [ "$mode" = rev ]; then
  A=$1; B=${2:-WORK}
  one() {  # <rev> <tag>
    if [ "$1" = WORK ]; then SRC=$PWD; else SRC=/tmp/ab_$2; rm -rf $SRC; git worktree add -f $SRC $1 >/dev/null 2>&1; fi
    build $SRC $PWD/gym_pomdp_amd/_lib/libpomdp_hip_$2.so
    if [ "$1" != WORK ]; then git worktree remove --force $SRC; fi
  }
  one $A a
  one $B b
else
  echo "usage: tools/ab_build.sh rev <revA> [revB]"; exit 1
fi
ls -la gym_pomdp_amd/_lib/*.so
