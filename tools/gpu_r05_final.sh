#!/bin/bash
# Round-5 end-state evidence (one gpurun call; every command under its own timeout, nothing reads stdin):
#   smoke, the default bench line, rocprofv3 --kernel-trace --stats of the bench command for both solvers, PMC FETCH_SIZE / WRITE_SIZE passes.
TAG=${1:-r05_final}
REPO=$(cd $(dirname $0)/.. && pwd); OUT=$REPO/gpurun_out; mkdir -p $OUT; cd $REPO
export CERES_HIP_PROBLEM_CACHE=/tmp/ceres_problem_cache
exec < /dev/null
echo "== smoke ($(date +%T))"
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1; tail -3 $OUT/smoke_$TAG.log | cut -c1-300
echo "== new tests ($(date +%T))"
timeout 600 python -m pytest tests/test_gpu_operators.py -m gpu -q -x --timeout 300 -k "fp32" 2>&1 | grep -v "^RCCL\|^HIP ver\|^ROCm\|^Hostname\|^Librccl" | tail -6 | tee $OUT/pytest_fp32_$TAG.log
echo "== bench ($(date +%T))"
timeout 600 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/bench_default_$TAG.json 2> $OUT/bench_default_$TAG.err
timeout 30 python - <<PY
import json
try:
    d = json.loads([l for l in open("$OUT/bench_default_$TAG.json").read().splitlines() if l.startswith("{")][-1])
    print({k: d[k] for k in ("value", "ms_per_step")}, "sx", d["roofline"]["frac"], d["roofline"]["avg_launch_ms"], "jtjx", d["roofline_jtjx"]["frac"], "oracle", (d.get("oracle_check") or {}).get("step_rel_diff_vs_oracle"), "cpu diff", d["cpu_baseline"]["step_rel_diff_vs_gpu"])
    print("fp32", d["extra"].get("fp32_tiles")); print("10M", {k: v for k, v in d["extra"].get("synthetic10M", {}).items() if k in ("steps_per_s", "sx_frac_hbm", "step_rel_diff_vs_oracle", "fp32_tiles")})
except Exception as ex:
    print("bench line unreadable:", ex)
PY
cd /tmp && export TMPDIR=/tmp
for SOLVER in iterative_schur cgnr; do
  echo "== rocprof $SOLVER ($(date +%T))"
  rm -rf /tmp/prof_$SOLVER
  timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_$SOLVER -o $SOLVER -- python $REPO/bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --both-solvers 0 --minimizer-iterations 0 --host-boundary-steps 0 --extra-synthetic10m 0 --extra-other-shapes 0 --extra-dense-cholesky 0 --solver $SOLVER > $OUT/bench_under_rocprof_${SOLVER}_$TAG.json 2> $OUT/rocprof_${SOLVER}_$TAG.err
  F=$(timeout 20 find /tmp/prof_$SOLVER -name "*kernel_stats.csv" | head -1)
  if [ -n "$F" ]; then cp "$F" $OUT/kernel_stats_${SOLVER}_venice_$TAG.csv; head -8 "$F" | cut -c1-170; else echo "no kernel_stats.csv"; tail -3 $OUT/rocprof_${SOLVER}_$TAG.err; fi
done
echo "== pmc ($(date +%T))"
for WL in venice1778 synthetic1M; do for C in FETCH_SIZE WRITE_SIZE; do
  rm -rf /tmp/pmc_$C
  timeout 300 rocprofv3 --pmc $C --kernel-trace --output-format csv -d /tmp/pmc_$C -o pmc -- python $REPO/tools/kernel_times.py $WL > /dev/null 2> $OUT/pmc_${C}_${WL}_$TAG.err
  F=$(timeout 20 find /tmp/pmc_$C -name "*counter_collection.csv" | head -1)
  if [ -n "$F" ]; then timeout 120 python - "$F" $C > $OUT/pmc_${C}_${WL}_$TAG.txt <<'PY'
import csv, sys, collections
rows = list(csv.DictReader(open(sys.argv[1])))
agg = collections.defaultdict(list)
for r in rows:
    if r.get("Counter_Name") == sys.argv[2]:
        agg[r["Kernel_Name"]].append(float(r["Counter_Value"]))
print("columns:", list(rows[0].keys()) if rows else None)
for k, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
    v2 = sorted(v)
    print(f"{k[:110]:110s} n={len(v):5d} mean={sum(v)/len(v):14.1f} median={v2[len(v2)//2]:14.1f} max={v2[-1]:14.1f}")
PY
  head -4 $OUT/pmc_${C}_${WL}_$TAG.txt | cut -c1-200; else echo "no counter csv for $C $WL"; fi
done; done
echo "== long cg ($(date +%T))"
cd $REPO; timeout 200 python tools/gpu_long_cg.py 30 2>/dev/null | tail -1 | tee $OUT/long_cg_$TAG.jsonl
echo "== done ($(date +%T))"
