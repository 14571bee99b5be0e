#!/bin/bash
# usage: bash scripts/exp/lr_sched_cost.sh [OUT]
# Price of a per-step optim.DeviceLR under hipGraph replay (scripts/exp/lr_sched_cost.py): the two
# variants alternated three times, a fresh process and a time limit of its own for every
# run, chained so that the first failure ends the script.  Appends to OUT (default: stdout only).
set -o pipefail
cd "$(dirname "$0")/../.." || exit 1
OUT=${1:-/dev/null}
mkdir -p "$(dirname "$OUT")"
run() { timeout -k 10 120 python -u scripts/exp/lr_sched_cost.py "$1" 2>&1 | grep "us/step" | tee -a "$OUT"; }
run none && run device_lr && run none && run device_lr && run none && run device_lr
