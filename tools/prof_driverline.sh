set -u
REPO=$(cd "$(dirname "$0")/.." && pwd); P=${PROF_OUT:-prof_out}; OUT=$REPO/$P/prof_r19_driverline; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- python3 $REPO/bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/trace.log 2> $OUT/trace.err
echo rc $?
cd $REPO && python tools/summarize_prof.py r19_driverline $P/summ; rm -rf $OUT/trace
