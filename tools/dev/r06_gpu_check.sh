#!/bin/bash
# Dev: new concurrency tests, the two-handle rounds, the whole GPU suite and a bench line in one GPU call.  Usage: tools/dev/r06_gpu_check.sh <output dir>
D=${1:?usage: $0 <output dir>}
mkdir -p "$D"
python -m pytest tests/test_concurrency.py -m gpu -x -q -s > "$D/concurrency.txt" 2>&1; tail -15 "$D/concurrency.txt"
python tools/dev/two_handles_diag.py --rounds 100 --max-dumps 2 --streams own > "$D/two_handles_own.log" 2>&1; grep "handle\|SUMMARY" "$D/two_handles_own.log" | tail -4
python -m pytest tests -m gpu -x -q > "$D/gpu_tests.txt" 2>&1; tail -3 "$D/gpu_tests.txt"
python bench.py --full > "$D/bench.json" 2> "$D/bench.err"; tail -c 700 "$D/bench.json"
