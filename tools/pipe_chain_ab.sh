#!/bin/bash
# Producer/consumer sweep (rotated roles, prioritized consumer) chained: the chain and pipe parity
# tests, then the 8-GPU slice: traces and alternating bench A/B of grouped+chain (default) vs
# pipe (separate launches) vs pipe+chain, with and without the one-rank P2P exchange.
set -e -o pipefail
O=gpurun_out/${1:-pchain}
mkdir -p $O
[ -n "$SKIP_TESTS" ] || { timeout -k 10 300 python -u -m pytest tests/test_gpu_chain.py tests/test_gpu_parity.py -k "chain or pipe" -x -q --timeout 200 --timeout-method thread > $O/pytest.txt 2>&1 || { tail -30 $O/pytest.txt; exit 1; }; tail -1 $O/pytest.txt; }
T="timeout -k 10 120 python3 tools/trace_probe.py --n-lam 62500"
FREI_HIP_LIB=abv/trace.so FREI_PIPE=4 $T 2>/dev/null > $O/t_pipe_chain.txt; echo "== pipe chain"; cat $O/t_pipe_chain.txt
FREI_HIP_LIB=abv/trace.so FREI_PIPE=4 FREI_CHAIN=0 $T 2>/dev/null > $O/t_pipe.txt; echo "== pipe"; cat $O/t_pipe.txt
B="python3 bench.py --full --n-lam 62500 --steps 40 --warmup 5 --rad-eq-max 1 --no-binning --no-cpu-baseline --no-c5 --no-per-species --no-chemistry"
for r in 1 2 3; do
  for cfg in "0 1" "4 0" "4 1"; do
    set -- $cfg
    FREI_PIPE=$1 FREI_CHAIN=$2 timeout -k 10 120 $B > $O/b_$1_$2_$r.json 2>/dev/null
    FREI_PIPE=$1 FREI_CHAIN=$2 timeout -k 10 120 $B --force-comm > $O/bp_$1_$2_$r.json 2>/dev/null
    python3 -c "import json; f=lambda n: json.load(open('$O/'+n+'_$1_$2_$r.json')); print('pipe $1 chain $2', $r, round(f('b')['ms_per_step']*1e3,2), 'us/iter; p2p', round(f('bp')['ms_per_step']*1e3,2))"
  done
done
