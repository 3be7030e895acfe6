#!/bin/bash
# One GPU-box session: parity tests, smoke, bench, rocprofv3 kernel stats (outputs in bench_out/).
set -o pipefail
cd "$(dirname "$0")/../.."; ROOT=$PWD
mkdir -p bench_out
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -x -v -m gpu --timeout 300 --timeout-method thread > bench_out/gpu_tests.log 2>&1 || { tail -40 bench_out/gpu_tests.log; exit 1; }
tail -3 bench_out/gpu_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > bench_out/smoke.log 2>&1 || { cat bench_out/smoke.log; exit 1; }
cat bench_out/smoke.log
timeout -k 10 400 python bench.py --full > bench_out/bench.json 2> bench_out/bench.err || { tail -20 bench_out/bench.err; exit 1; }
cat bench_out/bench.json
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d bench_out/prof -o run -- python3 bench.py --full --no-cpu-baseline > bench_out/prof_bench.json 2> bench_out/prof.err || { tail -20 bench_out/prof.err; exit 1; }
cat bench_out/prof_bench.json
find bench_out/prof -name "*stats*"
