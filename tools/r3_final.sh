#!/bin/bash
# What the driver runs at round end, rehearsed: the GPU suite, smoke(), the default bench line.
set -e
OUT=${OUT:-out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $OUT/r3zs_pytest.log 2>&1 || { tail -40 $OUT/r3zs_pytest.log; exit 1; }
tail -2 $OUT/r3zs_pytest.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
timeout -k 10 600 python bench.py --full > $OUT/r3zs_bench_default.json 2> $OUT/r3zs_bench_default.err || { tail -5 $OUT/r3zs_bench_default.err; exit 1; }
python3 -c "
import json
d=json.loads(open('$OUT/r3zs_bench_default.json').read().strip().splitlines()[-1]); r=d['roofline']
print(d['metric'], d['value'], d['unit'], d['ms_per_step'], 'steps', d['steps'], 'calls', d['config']['calls'], 'bound', r['bound'], r['frac'], 'sec8d', r['contract_sec8d']['frac'], 'cpu', d['cpu_baseline']['value'], d['cpu_baseline']['cores'], 'instrumented call', d['instrumented_call']['value'])"
timeout -k 10 300 python bench.py --full --config c1 --steps 8 --warmup 2 > $OUT/r3zs_bench_c1.json 2> $OUT/r3zs_bench_c1.err || { tail -5 $OUT/r3zs_bench_c1.err; exit 1; }
python3 -c "
import json
d=json.loads(open('$OUT/r3zs_bench_c1.json').read().strip().splitlines()[-1]); print('c1', d['value'], d['ms_per_step'], d['config']['pool_slots'], d['cpu_baseline']['full_frame'])"
timeout -k 10 500 python tools/parity_sweep.py > $OUT/r3zs_parity_sweep.log 2>&1 || { tail -5 $OUT/r3zs_parity_sweep.log; exit 1; }
tail -1 $OUT/r3zs_parity_sweep.log
