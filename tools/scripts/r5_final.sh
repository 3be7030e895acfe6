#!/bin/bash
# Round-5 evidence (GPU box): the GPU test suite, the driver-shaped bench line, and the same bench
# command under rocprofv3 --kernel-trace --stats (kernel summary for profiles/).
set -o pipefail
cd "$(dirname "$0")/../.."; ROOT=$PWD; mkdir -p bench_out; export TMPDIR=/tmp
tag=${1:-r5f}
timeout -k 10 700 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > bench_out/${tag}_tests.log 2>&1 \
  || { tail -20 bench_out/${tag}_tests.log; exit 1; }
tail -2 bench_out/${tag}_tests.log
timeout -k 10 600 python3 -u bench.py --full --steps 20 --warmup 5 > bench_out/${tag}_bench.json 2> bench_out/${tag}_bench.err || { tail -20 bench_out/${tag}_bench.err; exit 1; }
grep '^{' bench_out/${tag}_bench.json | tail -1 | cut -c1-240
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d bench_out/${tag}_prof -o p -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-pmc \
  > bench_out/${tag}_prof.log 2>&1 || { tail -20 bench_out/${tag}_prof.log; exit 1; }
find bench_out/${tag}_prof -name '*stats*' | head
