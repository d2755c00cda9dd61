#!/bin/bash
# one GPU-box visit: parity tests, bench, rocprofv3 kernel stats and HBM PMC passes (outputs under $OUT, default round_out/)
# usage: tools/gpu_round.sh TAG [steps...]   steps: tests bench prof pmc kbench  (default: all)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
OUT=${OUT:-$R/round_out}
TAG=${1:-r02}
shift
STEPS=${@:-tests bench prof pmc kbench}
mkdir -p $OUT
export TMPDIR=/tmp
has() { [[ " $STEPS " == *" $1 "* ]]; }
if has tests; then
  timeout -k 10 900 python -m pytest tests -m gpu -x -q > $OUT/tests_$TAG.log 2>&1
  echo "tests exit=$?" >> $OUT/tests_$TAG.log
  tail -3 $OUT/tests_$TAG.log
fi
if has bench; then
  timeout -k 10 400 python bench.py --full > $OUT/bench_$TAG.log 2>&1
  echo "bench exit=$?"; tail -1 $OUT/bench_$TAG.log | cut -c1-1500
fi
if has prof; then
  cd /tmp
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python3 $R/bench.py --full --steps 200 --warmup 20 --cpu-seconds 0 --no-anchor --no-live-traffic > $OUT/prof_$TAG.log 2>&1
  # (--no-anchor: `--stats` averages per kernel NAME and the anchor launches the same K1 / K3 instantiation on 10x the columns;
  #  tools/trace_by_grid.py splits a full run's trace by grid size instead.  --no-live-traffic: no rocprofv3 --pmc children
  #  inside a traced process -- the pmc step below measures the traffic on its own)
  echo "rocprof stats exit=$?"
  cd $R
fi
if has pmc; then
  cd /tmp
  N=${PMC_COLS:-35718}; ROT=${PMC_ROT:-2}
  timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch_$TAG -- python3 $R/tools/pmc_run.py $N $ROT > $OUT/pmc_fetch_$TAG.log 2>&1
  echo "pmc fetch exit=$?"
  timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write_$TAG -- python3 $R/tools/pmc_run.py $N $ROT > $OUT/pmc_write_$TAG.log 2>&1
  echo "pmc write exit=$?"
  cd $R && python tools/pmc_summary.py $OUT/pmc_fetch_$TAG $OUT/pmc_write_$TAG $N 268435456 $OUT/traffic_$TAG.json > $OUT/pmc_summary_$TAG.log 2>&1
  tail -30 $OUT/pmc_summary_$TAG.log
fi
if has kbench; then
  timeout -k 10 400 python tools/kbench.py --sizes ${KB_SIZES:-1024,2048,4096,8192,16384,35718,43566,348528} --cbs 0 > $OUT/kbench_sizes_$TAG.log 2>&1
  grep n= $OUT/kbench_sizes_$TAG.log
fi
