#!/bin/bash
# Round profile bundle (on the GPU box, from the repo root): rocprofv3 kernel-trace stats of the
# default bench, the per-launch layer table, and the PMC HBM-traffic passes (tools/pmc_traffic.sh).
# usage: bash tools/profile_round.sh <outdir>   (copy the summaries into profiles/ afterwards)
set -e
export TMPDIR=/tmp
O=${1:?usage: tools/profile_round.sh <outdir>}; mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_round -o run -- python3 bench.py --full --no-cpu-baseline > $O/prof_round.log 2>&1
timeout -k 10 200 python3 -u bench.py --full --no-cpu-baseline --layers > $O/layers_round.log 2>&1
bash tools/pmc_traffic.sh r50_mixed 3 256 > $O/pmc_round.log 2>&1
