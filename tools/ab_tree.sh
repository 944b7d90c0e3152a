#!/bin/bash
# tools/ab_tree.sh <tag> libA.so libB.so ...: the ordered count (--engine tree, config 4) with each library in turn, REPS times, on one box
TAG=$1; shift
cd $GRAFT_REPO_ROOT
O=${AB_OUT:-ab_out}/$TAG            # the bench lines (--full: each carries its digest check)
mkdir -p $O
for rep in $(seq 1 ${REPS:-2}); do
  for L in "$@"; do
    N=$(basename $L .so)
    DNAGPU_LIB_PATH=$PWD/$L timeout -k 10 300 python bench.py --engine tree --steps 5 --warmup 2 --full --no-cpu-baseline > $O/${N}_$rep.json 2> $O/${N}_$rep.err
    python - <<PY
import json
l=json.loads(open('$O/${N}_$rep.json').read().strip().splitlines()[-1])
p=l['phases_ms']
print('$N rep $rep: %.2f ms  %.1f G digest_ok=%s' % (l['ms_per_step'], l['value']/1e9, l.get('digest_ok')), {k:round(v,2) for k,v in p.items() if v>0.5})
PY
  done
done
