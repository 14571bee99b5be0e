#!/bin/bash
# Alternating pairs of bench.py on two built trees (default path A/B, profiles/ema_ab.txt section 1):
#
#   scripts/exp/bench_pairs.sh PARENT_TREE {convnet|resnet50} [PAIRS] > pairs.txt
#
# PARENT_TREE is a checkout of the parent commit with its own built extension; the other side is
# the tree this script lives in.  Each run is a fresh process under its own time limit; the first
# failure ends the script.  One line per run: "pair I SIDE <bench.py's JSON line>".
set -o pipefail
here=$(cd "$(dirname "$0")/../.." && pwd)
parent=$(cd "$1" && pwd) || exit 2
which=${2:-convnet}
pairs=${3:-5}
if [ "$which" = convnet ]; then
  args="--gpus 1 --steps 2000 --warmup 50"; limit=150
else
  args="--gpus 1 --model resnet50 --steps 20 --warmup 5"; limit=240
fi
for i in $(seq 1 "$pairs"); do
  for side in parent new; do
    if [ $side = parent ]; then dir=$parent; else dir=$here; fi
    line=$(cd "$dir" && timeout -k 10 $limit python bench.py $args 2>/dev/null | grep '^{' | tail -1)
    if [ -z "$line" ]; then echo "pair $i $side FAILED" >&2; exit 1; fi
    echo "pair $i $side $line"
  done
done
