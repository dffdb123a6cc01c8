#!/bin/bash
# rocprofv3 kernel trace of 20 graph-replayed sampling steps -> step table (and the bench line with its
# roofline leg, which tools/reconcile.py compares with the table).
# usage: TAG=x [OUT=dir] bash tools/steptable.sh
TAG=${TAG:-st}
OUT=${OUT:-build/steptable}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o run -- python3 -u bench.py --steps 20 --warmup 3 --full --no-parity --no-cpu-baseline > $OUT/${TAG}_prof.log 2>&1
rc=$?; echo prof_rc=$rc; [ $rc -ne 0 ] && { tail -5 $OUT/${TAG}_prof.log; exit $rc; }
grep -o '"ms_per_step": [0-9.]*' $OUT/${TAG}_prof.log
python3 tools/step_table.py $OUT/${TAG}_prof 20 --json $OUT/${TAG}_step_table.json > $OUT/${TAG}_step_table.txt 2>&1
cut -c1-120 $OUT/${TAG}_step_table.txt
