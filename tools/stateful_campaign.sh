#!/bin/bash
# Stateful fuzz campaign on the GPU box: tests/test_stateful_gpu.py (random interleavings of every mutator and every query
# against the host model) under a range of PGX_STATEFUL_SEED values -- one pytest process per value, each under its own
# time limit.  Steps that are a multiple of 4 keep every (mutator, cache query) pair in each value's sequences.
# The loop STOPS at the first value that does not pass: after a mismatch the next step is to replay it on the host
# (PGX_STATEFUL_OPS), and after a fault nothing more may start on that GPU.
# usage: tools/stateful_campaign.sh <first> <last> <step> [outfile]
first=${1:-4}; last=${2:-400}; step=${3:-4}; out=${4:-build/stateful_campaign.txt}
mkdir -p "$(dirname "$out")"; : > "$out"
log=$(mktemp)
for s in $(seq $first $step $last); do
  PGX_STATEFUL_SEED=$s timeout -k 10 600 python -m pytest tests/test_stateful_gpu.py -m gpu -x -q > "$log" 2>&1
  rc=$?
  echo "PGX_STATEFUL_SEED=$s: rc=$rc $(tail -1 "$log")" | tee -a "$out"
  if [ $rc -ne 0 ]; then
    grep -E "^E " "$log" | head -40 | cut -c1-4000 | tee -a "$out"
    echo "campaign $first..$last step $step: STOPPED at PGX_STATEFUL_SEED=$s (rc=$rc)" | tee -a "$out"
    rm -f "$log"
    exit $rc
  fi
done
rm -f "$log"
echo "campaign $first..$last step $step: CLEAN" | tee -a "$out"
