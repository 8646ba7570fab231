#!/bin/bash
# The four bench lines kept under profiles/ (GPU box):   bash tools/bench_lines.sh <tag>
TAG=${1:-lines}
cd $GRAFT_REPO_ROOT
O=${OUT_DIR:-out}/$TAG; mkdir -p $O
timeout 600 python bench.py --full > $O/bench.json 2> $O/bench.err
timeout 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $O/bench_driver_window.json 2>> $O/bench.err
timeout 300 python bench.py --full --path two-launch --no-cpu-baseline > $O/bench_two_launch.json 2>> $O/bench.err
timeout 300 python bench.py --full --workload c5 --no-cpu-baseline > $O/bench_c5.json 2>> $O/bench.err
for f in bench bench_driver_window bench_two_launch bench_c5; do python -c "import json,sys; d=json.loads(open('$O/$f.json').read().strip().splitlines()[-1]); r=d['roofline']; print('$f', d['value'], d['ms_per_step'], r['frac'], r.get('traffic'), (d.get('api_trainer') or {}).get('value'))"; done
