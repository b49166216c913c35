# Alternate full bench.py runs between two library builds on one box (A B A B ...).
#   bash tools/ab_bench.sh LIB_A LIB_B ROUNDS OUTDIR [bench args...]
set -e
A=$1; B=$2; R=$3; OUT=$4; shift 4
mkdir -p $OUT
for r in $(seq 1 $R); do
  FREI_HIP_LIB=$A timeout -k 10 200 python3 bench.py --full --no-cpu-baseline "$@" > $OUT/A_$r.json
  FREI_HIP_LIB=$B timeout -k 10 200 python3 bench.py --full --no-cpu-baseline "$@" > $OUT/B_$r.json
done
