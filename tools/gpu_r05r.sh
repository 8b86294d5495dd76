#!/bin/bash
cd $(dirname $0)/..; OUT=${OUT:-$(pwd)/out}; mkdir -p $OUT
export CERES_HIP_PROBLEM_CACHE=/tmp/ceres_problem_cache
timeout 1500 python -m pytest tests -m gpu -q --timeout 900 2>&1 | grep -v "^RCCL\|^HIP ver\|^ROCm\|^Hostname\|^Librccl" | tail -12 | tee $OUT/pytest_all_r05r.log
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/prof_r05r; timeout 600 rocprofv3 --kernel-trace --stats -d /tmp/prof_r05r -o p -- python $OLDPWD/bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --both-solvers 0 --minimizer-iterations 0 --host-boundary-steps 0 --extra-synthetic10m 0 --extra-other-shapes 0 --extra-dense-cholesky 0 > $OUT/bench_under_rocprof_r05r.json 2>/dev/null
F=$(find /tmp/prof_r05r -name "*kernel_stats.csv" | head -1); cp $F $OUT/kernel_stats_r05r.csv; head -14 $F | cut -c1-160
