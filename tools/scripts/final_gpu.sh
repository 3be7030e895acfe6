#!/bin/bash
# End-of-round evidence: parity tests, smoke, bench, rocprofv3 stats, PMC traffic passes.
set -o pipefail
cd "$(dirname "$0")/../.."; ROOT=$PWD; mkdir -p bench_out
tools/scripts/round_gpu.sh > bench_out/round.log 2>&1 || { tail -30 bench_out/round.log; exit 1; }
tail -4 bench_out/gpu_tests.log
tools/scripts/pmc.sh || { echo "pmc failed"; exit 1; }
python tools/scripts/make_pmc_json.py bench_out/pmc_fetch/p_counter_collection.csv bench_out/pmc_write/p_counter_collection.csv bench_out/pmc.json
find bench_out/prof bench_out/prof1 -name "*stats*"
cat bench_out/bench.json
