#!/bin/bash
# full verification of the tree: the GPU suite, smoke(), the full bench line (every leg)
# usage (from the repo root): scripts/gpu_check.sh <output dir>
# A step that times out or dies on a signal ends the check: nothing more is started on the GPU after it.
O=${1:?usage: scripts/gpu_check.sh <output dir>}
mkdir -p "$O"
stop_on_crash() { case $1 in 124|134|137|139) echo "$2 exited with $1: stopping" | tee -a "$O/check_stopped.log"; exit "$1";; esac; }
timeout 1500 python -m pytest tests -m gpu -q -x > "$O/check_gpu_tests.full.log" 2>&1; rc=$?
tail -6 "$O/check_gpu_tests.full.log" > "$O/check_gpu_tests.log"; stop_on_crash $rc pytest
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O/check_smoke.log" 2>&1; rc=$?; echo "smoke rc=$rc" >> "$O/check_smoke.log"; stop_on_crash $rc smoke
MPCQP_BENCH_LEGS="$O/check_bench_full_legs.json" timeout 900 python bench.py --full > "$O/check_bench_full.json" 2> "$O/check_bench_full.err"; echo "bench rc=$?" >> "$O/check_bench_full.err"
cat "$O/check_gpu_tests.log"; tail -3 "$O/check_smoke.log"; tail -2 "$O/check_bench_full.err"; cut -c1-600 "$O/check_bench_full.json"
