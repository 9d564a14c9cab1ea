#!/bin/bash
# One GPU session: the secondary config bench lines (bench_configs.py), then three rocprofv3 PMC
# passes over the headline bench with its other lines (bench.py --full: SQ occupancy/VALU, HBM
# reads, HBM writes), each pass its own run.  Every GPU step has its own time limit; a fault /
# abort / time limit ends the script (exit 1 = an ordinary Python error, reported and the next
# step still runs).  Outputs go under $OUT (default prof_out/).
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-prof_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
step() {
  local lim=$1; shift
  echo "== $*" >&2
  timeout -k 10 "$lim" "$@"
  local rc=$?
  if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "stopping: rc=$rc from: $*" >&2; exit $rc; fi
  return 0
}
step 400 python3 -u bench_configs.py --configs c2,c4 > $OUT/bench_c2_c4.json 2> $OUT/bench_c2_c4.err
step 500 python3 -u bench_configs.py --configs c5 --steps 1 > $OUT/bench_c5.json 2> $OUT/bench_c5.err
step 60 rocprofv3 -L > $OUT/pmc_list.txt 2>&1
SQ="SQ_WAVES SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_SALU SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_ANY"
step 180 rocprofv3 --pmc $SQ --output-format csv -d $OUT/pmc_sq -o pmc -- python3 bench.py --full --no-cpu --steps 1 --warmup 0 > $OUT/pmc_sq.log 2>&1
step 180 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o pmc -- python3 bench.py --full --no-cpu --steps 1 --warmup 0 > $OUT/pmc_fetch.log 2>&1
step 180 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o pmc -- python3 bench.py --full --no-cpu --steps 1 --warmup 0 > $OUT/pmc_write.log 2>&1
python3 tools/pmc_summary.py $OUT/pmc_summary.json $OUT/pmc_sq $OUT/pmc_fetch $OUT/pmc_write > $OUT/pmc_summary.txt 2>&1
echo done >&2
