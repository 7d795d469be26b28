#!/bin/bash
# Everything profiles/<tag>_* of a round is made of, in one GPU-box job:  gpurun --timeout 2400 -- 'bash tools/round_profiles.sh r06'
#   <tag>_kernel_stats.csv, <tag>_pmc.json            inference step (tools/profile_round.sh)
#   <tag>_train_kernel_stats.csv, <tag>_train_pmc.json training step (tools/tools_train_profile.sh, tools/profile_train_pmc.sh)
#   <tag>_bench_default.json                           the default bench command's full result (--full --details inline)
TAG=${1:-r06}
EG_OUT=${EG_OUT:-tool_out}                 # results folder (the scripts that call each other share it)
export TMPDIR=/tmp
cd /tmp && cd $GRAFT_REPO_ROOT
mkdir -p $EG_OUT/profiles
bash tools/profile_round.sh $TAG > $EG_OUT/profiles/${TAG}_profile_round.log 2>&1
bash tools/profile_train_pmc.sh $TAG > $EG_OUT/profiles/${TAG}_profile_train_pmc.log 2>&1
bash tools/tools_train_profile.sh 32 > $EG_OUT/profiles/${TAG}_train_profile.txt 2>&1
cp $EG_OUT/profiles/train_kernel_stats.csv $EG_OUT/profiles/${TAG}_train_kernel_stats.csv
# the PMC summaries have to be where bench.py looks for them before the bench run below reports `traffic`
cp $EG_OUT/profiles/${TAG}_pmc.json $EG_OUT/profiles/${TAG}_train_pmc.json profiles/ 2>/dev/null
timeout 1200 python bench.py --full --details inline > $EG_OUT/profiles/${TAG}_bench_default.json 2> $EG_OUT/profiles/${TAG}_bench_default.log
tail -c 600 $EG_OUT/profiles/${TAG}_bench_default.json; tail -12 $EG_OUT/profiles/${TAG}_profile_train_pmc.log
