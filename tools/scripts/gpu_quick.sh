#!/bin/bash
# GPU tests (optionally a subset: pass pytest args) then the default bench line.
set -o pipefail
cd "$(dirname "$0")/../.."; ROOT=$PWD; mkdir -p bench_out; export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -x -v -m gpu --timeout 300 --timeout-method thread "$@" > bench_out/gpu_tests.log 2>&1 || { tail -40 bench_out/gpu_tests.log; exit 1; }
tail -3 bench_out/gpu_tests.log
timeout -k 10 400 python bench.py --full --no-cpu-baseline > bench_out/bench.json 2> bench_out/bench.err || { tail -20 bench_out/bench.err; exit 1; }
cat bench_out/bench.json
