#!/bin/bash
# round 5: the full bench line once more, with this library's counter summary in profiles/ (traffic, hbm_side counters filled in);
# the line and its log go to $OUT
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-$TMPDIR/r05_bench}; mkdir -p "$OUT"
timeout -k 10 400 python3 bench.py --full > "$OUT/r05_bench_final.json" 2> "$OUT/r05_bench_final.err" || exit 1
python3 -c "
import json, sys; b=json.load(open(sys.argv[1])); r=b['roofline']
print(b['value'], r['frac'], r.get('traffic'), r.get('mfma_busy'), r.get('useful_over_executed'))
print(json.dumps(r['hbm_side'])[:1500])" "$OUT/r05_bench_final.json"
