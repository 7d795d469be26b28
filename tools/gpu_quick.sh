#!/bin/bash
# quick GPU check of a change: selected tests, then the batch-1 graphed training step and the batch-32 step
#   gpurun -- 'bash tools/gpu_quick.sh <tag> "<pytest -k expression>"'
tag=${1:-q}; expr=${2:-coord}
EG_OUT=${EG_OUT:-tool_out}                 # results folder (the scripts that call each other share it)
cd "$GRAFT_REPO_ROOT" || exit 1
mkdir -p $EG_OUT
timeout 1200 python -m pytest tests -x -q -m gpu -k "$expr" > $EG_OUT/${tag}_tests.log 2>&1
tail -15 $EG_OUT/${tag}_tests.log
timeout 240 python bench.py --mode train --full --batch 1 --steps 50 --warmup 5 --no-other-configs --details inline 2>/dev/null | python -c "
import sys, json
d = json.loads(sys.stdin.read().strip().splitlines()[-1])
print('B=1 train eager ms', d['ms_per_step'], 'graphed', (d.get('hip_graph_replay') or {}).get('ms_per_step'))"
timeout 240 python bench.py --mode train --full --batch 32 --steps 30 --warmup 5 --no-other-configs --details inline 2>/dev/null | python -c "
import sys, json
d = json.loads(sys.stdin.read().strip().splitlines()[-1])
print('B=32 train eager ms', d['ms_per_step'], 'graphed', (d.get('hip_graph_replay') or {}).get('ms_per_step'))"
