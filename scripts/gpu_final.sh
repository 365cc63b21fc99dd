#!/bin/bash
# Round-end verification on one GPU: parity suite, smoke(), default bench line, rocprofv3 kernel stats + trace.
set -e
export TMPDIR=/tmp && cd "$(dirname "$0")/.."
OUT=${OUT:-prof_out}  # where every output of this script goes (kept out of git)
mkdir -p $OUT
TAG=${TAG:-fin}
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/t_$TAG.log 2>&1 || { tail -40 $OUT/t_$TAG.log; exit 1; }
tail -1 $OUT/t_$TAG.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke_$TAG.log 2>&1 || { tail -20 $OUT/smoke_$TAG.log; exit 1; }
tail -1 $OUT/smoke_$TAG.log
timeout -k 10 300 python bench.py --full >$OUT/b_$TAG.log 2>&1 || { tail -20 $OUT/b_$TAG.log; exit 1; }
tail -1 $OUT/b_$TAG.log | cut -c1-400
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- python3 bench.py --steps 10 --warmup 3 --no-cpu-baseline > $OUT/prof_$TAG.log 2>&1 || { tail -20 $OUT/prof_$TAG.log; exit 1; }
python scripts/trace_summary.py $OUT/prof_$TAG/run_kernel_trace.csv --top 40 > $OUT/ts_$TAG.txt
head -8 $OUT/ts_$TAG.txt
