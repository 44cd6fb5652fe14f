#!/bin/bash
# One GPU run: GPU tests, the bench line of every BASELINE workload (the full line of the default one), then the profiles.
# Everything lands in $OUT (default out/).   usage: scripts/gpu_round.sh r02 [skip-tests]
R=${1:-r02}
export OUT=$(realpath -m "${OUT:-out}")
mkdir -p $OUT
if [ "${2:-}" != skip-tests ]; then
  timeout 1500 python -m pytest tests -m gpu -x -q > $OUT/${R}_pytest_gpu.log 2>&1; echo "pytest rc=$?" | tee -a $OUT/${R}_pytest_gpu.log
  tail -5 $OUT/${R}_pytest_gpu.log
fi
timeout 900 python bench.py --full > $OUT/${R}_bench_default.json 2> $OUT/${R}_bench_default.err; echo "bench rc=$?"; cat $OUT/${R}_bench_default.json | cut -c1-1500
for WL in pile8k mixed32k islands256k chains16k ragdolls1k polyheap32k; do
  case $WL in islands256k) A="--steps 60 --warmup 10";; polyheap32k) A="--steps 100 --warmup 10";; *) A="";; esac
  timeout 600 python bench.py --workload $WL $A --north-star none --other-arithmetic-steps 0 --no-cpu-baseline > $OUT/${R}_bench_$WL.json 2> $OUT/${R}_bench_$WL.err; echo "$WL rc=$?"; cut -c1-400 $OUT/${R}_bench_$WL.json
done
timeout 2400 bash scripts/profile_round.sh $R pile32k pile8k mixed32k islands256k chains16k ragdolls1k polyheap32k > $OUT/${R}_profile.log 2>&1; echo "profile rc=$?"
