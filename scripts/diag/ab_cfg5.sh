#!/bin/bash
# usage (GPU box): scripts/diag/ab_cfg5.sh <lib.so> [<lib.so> ...]   -- cfg-5 bench of several builds of the library side by side
# (the other path and the parity setting are legs of a --full run; they are read from its full record)
legs=$(mktemp); trap 'rm -f "$legs"' EXIT
for b in 256 512 1024; do for lib in "$@"; do MPCQP_BENCH_LEGS=$legs python scripts/bench_with_lib.py $lib --workload cfg5 --full --no-cpu-baseline --batch $b > /dev/null || exit 1; python - "$legs" "$lib" $b <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print(sys.argv[2], sys.argv[3], "loop %.0f stepwise %.0f parity %.0f  iters %.2f/%.2f  frac %.2f" % (d["value"], d["other_path"]["value"], d["parity_setting"]["value"], d["mean_admm_iters"], d["parity_setting"]["mean_admm_iters"], d["roofline"]["frac"]))
PY
done; done
