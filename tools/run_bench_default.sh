#!/bin/bash
# The driver's default bench line with everything --full adds (C2, one GPU, roofline, transfers, CPU baseline) and a functional two-rank run
# on the same GPU:  bash tools/run_bench_default.sh [output folder, default bench_out]
O=${1:-bench_out}
mkdir -p "$O"
if [ -z "$SKIP_DEFAULT" ]; then
timeout 900 python bench.py --full > "$O/bench_default.json" 2> "$O/bench_default.err"; echo "bench rc=$?"
python -c "
import json, sys; d=json.load(open(sys.argv[1])); print(d['value'], d['ms_per_step'], d['iterations_per_step'], d['transfers']['frac_of_hbm_peak'], d['transfers']['per_step_ms'], d['roofline']['frac'], d['cpu_baseline']['value'], d['cpu_baseline']['fair_value'])" "$O/bench_default.json"
fi
timeout 900 python bench.py --share-gpu --gpus 2 --steps 2 --warmup 1 --no-cpu --cells 40 2> "$O/bench_2r.err" | tail -1 > "$O/bench_2r.json"
python -c "
import json, sys; d=json.load(open(sys.argv[1])); print('2 ranks on one GPU:', d['value'], d['ms_per_step'], d['n_gpus'], d['config']['parallelism'][:80], d['comm_per_step_rank0'])" "$O/bench_2r.json"
