#!/bin/bash
# Round 6, last GPU check at the final code: smoke(), the whole -m gpu suite, and the N > 1 code
# path's one-rank rehearsal (bench.py --sharded: batched shards + the RCCL gather on a one-rank group).
set -o pipefail
cd "$(dirname "$0")/../.."; ROOT=$PWD; mkdir -p bench_out; export TMPDIR=/tmp
timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke()" > bench_out/r6l_smoke.log 2>&1 || { tail -20 bench_out/r6l_smoke.log; exit 1; }
tail -1 bench_out/r6l_smoke.log
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > bench_out/r6l_tests.log 2>&1 \
  || { tail -30 bench_out/r6l_tests.log; exit 1; }
tail -1 bench_out/r6l_tests.log
timeout -k 10 300 python -u bench.py --full --sharded --steps 20 --no-cpu-baseline --no-pmc --no-legs --no-config2 > bench_out/r6l_sharded.json 2> bench_out/r6l_sharded.err \
  || { tail -20 bench_out/r6l_sharded.err; exit 1; }
grep '^{' bench_out/r6l_sharded.json | tail -1 | cut -c1-220
