# round-end evidence: full GPU suite, bench line + kernel trace + frame trace + traffic counters, PMC pass over the kernels,
# the other BASELINE configurations
#   tools/run_final.sh <tag> [dir]     -> <dir>/<tag>/, dir defaults to results
TAG=${1:-r2z}
DIR=${2:-results}
OUT=$DIR/$TAG
mkdir -p $OUT
(timeout 1100 python -m pytest tests -m gpu -q --durations=10 > $OUT/pytest.log 2>&1; echo "pytest rc=$?" >> $OUT/pytest.log); tail -16 $OUT/pytest.log
timeout 900 bash tools/profile_round.sh $TAG $DIR > $OUT/profile_round.log 2>&1; tail -30 $OUT/profile_round.log
export TMPDIR=/tmp
timeout 300 bash tools/pmc_ops.sh $OUT/${TAG}_pmc_ops.txt > $OUT/pmc_ops.log 2>&1; tail -2 $OUT/pmc_ops.log
for cfgs in "256 256 1 12" "512 768 2 24" "512 512 4 16" "576 1024 2 40"; do set -- $cfgs
  timeout 300 python bench.py --height $1 --width $2 --denoise-steps $3 --window $4 --steps 20 --warmup 5 --full --no-cpu-baseline --breakdown 0 > $OUT/bench_$1x$2_n$3_L$4.json 2>> $OUT/bench_other.err
  python -c "
import json
d=json.loads(open('$OUT/bench_$1x$2_n$3_L$4.json').read().strip().splitlines()[-1]); print(d['config']['workload'][:60], d['value'], d['ms_per_step'], d['config']['kv_cache_GB_per_stream'], (d.get('whole_frame') or {}).get('frames_per_s'))"
done
timeout 200 python tools/midas_time.py 1 > $OUT/${TAG}_midas_time.json 2>> $OUT/bench_other.err; cat $OUT/${TAG}_midas_time.json
