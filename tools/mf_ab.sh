#!/bin/bash
# A/B of the element-chunk operator's runtime knobs (run on the GPU box): tools/mf_probe.py with the default settings
# and with each environment variable NAME=VALUE named.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
O=${OUT:-gpurun_out/mf_ab}
mkdir -p $O
ARGS=${MF_ARGS:-"--n 119 --no-assembled --iters 50"}
timeout -k 10 150 python3 tools/mf_probe.py $ARGS > $O/default.log 2>&1 || exit $?
echo "default $(tail -1 $O/default.log)"
for v in "$@"; do   # NAME=VALUE
  env "$v" timeout -k 10 150 python3 tools/mf_probe.py $ARGS > $O/env_$v.log 2>&1 || exit $?
  echo "$v $(tail -1 $O/env_$v.log)"
done
