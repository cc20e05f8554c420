#!/bin/bash
# IMAGENT_GRAM_T A/B: alternating `python bench.py` (defaults) pairs of a built checkout of the parent commit and
# this tree, then one switch-off run of this tree. Every run has its own time limit; stops at the first failure.
# Usage (GPU box, from this tree's root): bash scripts/runs/gram_t_ab.sh PARENT_DIR [PAIRS] [OUT_DIR]
set -o pipefail
P=${1:?built checkout of the parent commit}
N=${2:-5}
O=$(realpath -m ${3:-bench_out/gram_t_ab})
R=$(pwd)
mkdir -p $O
run() {  # tag dir env...
    local tag=$1 dir=$2; shift 2
    (cd $dir && env "$@" timeout -k 10 240 python -u bench.py > $O/$tag.log 2>&1) || { tail -5 $O/$tag.log; exit 1; }
    echo "$tag $* $(grep -o '"value": [0-9.]*' $O/$tag.log | tail -1)" | tee -a $O/summary.txt
}
for i in $(seq 1 $N); do
    run parent_$i $P IMAGENT_X=0
    run pr_$i $R IMAGENT_GRAM_T=1
done
run pr_off $R IMAGENT_GRAM_T=0
