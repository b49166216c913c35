# Round-end measurement on one MI355X: PMC traffic + VALU passes, the bench line, and the
# rocprofv3 kernel-trace stats of the same command.  Outputs under $1 (default bench_out/final).
set -e
O=${1:-bench_out/final}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
B="python3 bench.py --full --steps 10 --warmup 1 --rad-eq-max 1 --no-cpu-baseline --no-binning --no-c5"
timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -o run -- $B > $O/pmc_fetch.log 2>&1
timeout -s KILL 120 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -o run -- $B > $O/pmc_write.log 2>&1
timeout -s KILL 120 rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_sq -o run -- $B > $O/pmc_sq.log 2>&1
python3 tools/pmc_traffic.py $O/pmc_fetch $O/pmc_write profiles/traffic_sweep.json
python3 tools/pmc_valu.py $O/pmc_sq profiles/valu_sweep.json
cp profiles/traffic_sweep.json profiles/valu_sweep.json $O/
timeout -k 10 400 python3 bench.py --full > $O/bench.json 2> $O/bench.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o run -- python3 bench.py --full --no-cpu-baseline > $O/bench_under_rocprof.json 2> $O/bench_under_rocprof.err
# per-GPU slice sizes of the 2/4/8-GPU runs on one GPU (sweep + fixed per-sweep costs)
for n in 250000 125000 62500; do
  timeout -k 10 120 python3 bench.py --full --n-lam $n --steps 20 --no-binning --no-cpu-baseline --no-c5 > $O/bench_n$n.json 2>/dev/null
done
# per-sweep timeline (kernel durations and gaps) at the 8-GPU slice size
timeout -k 10 120 rocprofv3 --kernel-trace --output-format csv -d $O/prof_n62500 -o run -- python3 bench.py --full --n-lam 62500 --steps 20 --rad-eq-max 1 --no-binning --no-cpu-baseline --no-c5 > $O/bench_n62500_under_rocprof.json 2>/dev/null
python3 tools/timeline.py $O/prof_n62500/run_kernel_trace.csv > $O/timeline_n62500.txt
python3 tools/timeline.py $O/prof/run_kernel_trace.csv > $O/timeline_n500000.txt
