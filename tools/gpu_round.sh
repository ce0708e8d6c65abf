#!/bin/bash
# One GPU-box session: the -m gpu suite (optionally a subset), then (if the suite ended normally: all passed or
# assertion failures only) the full bench line.  Usage: [OUT=dir] tools/gpu_round.sh TAG [pytest selection...]
# Outputs: $OUT/gputest_TAG.txt, $OUT/bench_TAG.json (+ .log); OUT defaults to bench_out
TAG=$1; shift
SEL=${@:-tests}
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 1000 python -u -m pytest $SEL -m gpu -q -p no:cacheprovider --timeout 300 --timeout-method thread \
  > $OUT/gputest_$TAG.txt 2>&1
rc=$?
tail -3 $OUT/gputest_$TAG.txt
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "pytest rc=$rc: stopping"; exit $rc; fi
if [ -n "$NOBENCH" ]; then exit $rc; fi
timeout -k 10 600 python -u bench.py --full > $OUT/bench_$TAG.log 2>&1
brc=$?
tail -1 $OUT/bench_$TAG.log > $OUT/bench_$TAG.json
echo "bench rc=$brc"; head -c 600 $OUT/bench_$TAG.json; echo
exit $brc
