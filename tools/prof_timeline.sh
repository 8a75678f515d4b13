#!/bin/bash
# GPU timeline of one bench step (tools/rocpd_timeline.py) on the GPU box -> stdout
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
cd /tmp && export TMPDIR=/tmp
TL=$(mktemp -d)
rocprofv3 --kernel-trace -d $TL -o tl -- python $ROOT/bench.py --full --steps 100 --warmup 10 --no-cpu-baseline --no-query-extra --no-loglinear-extra "$@" > /dev/null 2>&1
cd $ROOT
python tools/rocpd_timeline.py $(find $TL -name "*.db" | head -1) ${ANCHOR:-vs_gather_mean} 60
rm -rf $TL
