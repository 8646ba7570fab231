#!/bin/bash
# One GPU visit: tests, bench line, rocprofv3 kernel stats, optional SQ counters.   bash tools/gpu_round.sh <tag> [notest] [nopmc]
TAG=${1:-x}
cd $GRAFT_REPO_ROOT
mkdir -p gpurun_out/$TAG
ROOT=$PWD; O=$ROOT/${OUT_DIR:-out}/$TAG; mkdir -p $O   # the bench lines and their kernel stats
if [[ "$*" != *notest* ]]; then
  timeout 1500 python -m pytest tests -m gpu -x -q > gpurun_out/$TAG/pytest.log 2>&1; echo "pytest rc=$?"; tail -5 gpurun_out/$TAG/pytest.log
fi
timeout 600 python bench.py --full > $O/bench.json 2> $O/bench.err; echo "bench rc=$?"; tail -c 1500 $O/bench.json
timeout 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $O/bench_driver_window.json 2>> $O/bench.err; echo
(cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --kernel-trace --stats -d $O/prof -- python $ROOT/bench.py --full --no-cpu-baseline --no-kernel-timing --no-api-trainer > $O/prof.log 2>&1)
DB=$(ls -t $O/prof/*/*_results.db 2>/dev/null | head -1)
[ -n "$DB" ] && python tools/rocpd_summary.py $DB > $O/kernel_stats.txt && head -8 $O/kernel_stats.txt
timeout 300 python bench.py --full --path two-launch --no-cpu-baseline > $O/bench_two_launch.json 2>> $O/bench.err
timeout 300 python bench.py --full --workload c5 --no-cpu-baseline > $O/bench_c5.json 2>> $O/bench.err
for f in bench_two_launch bench_c5; do python -c "import json,sys; d=json.loads(open('$O/$f.json').read().strip().splitlines()[-1]); print('$f', d['value'], d['ms_per_step'], d['config']['loop'])"; done
if [[ "$*" != *nopmc* ]]; then
  timeout 900 bash tools/pmc_sq.sh 256 $TAG > gpurun_out/$TAG/pmc_sq.txt 2>&1; tail -60 gpurun_out/$TAG/pmc_sq.txt
  timeout 600 bash tools/pmc_traffic.sh > gpurun_out/$TAG/pmc_traffic.txt 2>&1; tail -8 gpurun_out/$TAG/pmc_traffic.txt; cp gpurun_out/pmc/tick_traffic.json gpurun_out/$TAG/traffic.json
fi
