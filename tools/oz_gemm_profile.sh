# k_oz_gemm's profile for one library build (dev tool): rocprofv3 kernel trace of the single-stream
# bench, then counter passes of one evaluation, each in a run of its own (counters are never
# combined with tracing); tools/oz_gemm_summary.py reduces both to the int8 kernel's launches.
# Writes $OUT (default bench_out/) kernel_stats_TAG.csv, oz_trace_TAG.json, oz_pmc_TAG.json.
# usage: bash tools/oz_gemm_profile.sh TAG LIB
set -o pipefail
tag=$1
export GPEMU_LIB=$2
export TMPDIR=/tmp
O=${OUT:-bench_out}
mkdir -p $O
stop() { echo "step failed: $1 (exit $2)"; exit $2; }
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_$tag -o b -- \
  python3 bench.py --gpus 1 --steps 6 --warmup 2 --concurrent 1 --no-cpu-baseline --no-other-configs --no-rowblock \
  > $O/bench_prof_$tag.json 2> $O/bench_prof_$tag.err || stop trace $?
tail -1 $O/bench_prof_$tag.json | cut -c1-300
cp "$(find $O/trace_$tag -name '*kernel_stats.csv' | head -1)" $O/kernel_stats_$tag.csv || stop stats $?
python3 tools/oz_gemm_summary.py trace $O/trace_$tag $O/oz_trace_$tag.json || stop summary $?
rm -rf $O/trace_$tag
i=0
for ctrs in "SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_BUSY_CYCLES" "SQ_WAIT_INST_LDS SQ_INSTS_VALU SQ_INSTS_MFMA" "TCC_HIT_sum TCC_MISS_sum" "FETCH_SIZE"; do
  timeout -k 10 200 rocprofv3 --pmc $ctrs --output-format csv -d $O/pmc${i}_$tag -o r -- \
    python3 tools/prof_objective.py 16384 10 1 > $O/pmc${i}_$tag.log 2>&1
  rc=$?
  case $rc in
    0) ;;
    124|134|137|139) stop "pmc $ctrs" $rc ;;
    *) echo "pmc pass '$ctrs' refused (exit $rc):"; tail -3 $O/pmc${i}_$tag.log; rm -rf $O/pmc${i}_$tag ;;
  esac
  i=$((i + 1))
done
python3 tools/oz_gemm_summary.py pmc $O/pmc?_$tag $O/oz_pmc_$tag.json || stop pmcsummary $?
rm -rf $O/pmc?_$tag
