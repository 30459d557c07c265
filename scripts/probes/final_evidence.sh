#!/bin/bash
# Runs ON THE GPU BOX: end-of-round evidence in one call (tests, smoke, profiles, bench lines, parity report).  TAG = round tag,
# OUT = directory for the evidence files.
TAG=${1:-r03}
OUT=${OUT:?set OUT to the directory for the evidence files}
cd $GRAFT_REPO_ROOT
mkdir -p "$OUT"
python -m pytest tests -m gpu -q 2>&1 | tail -3
python __graft_entry__.py smoke 2>&1 | tail -3
bash scripts/collect_profiles.sh $TAG 2>&1 | tail -3
bash scripts/collect_secondary.sh $TAG > $OUT/secondary_$TAG.log 2>&1
cd $GRAFT_REPO_ROOT
python bench.py --full > $OUT/bench_${TAG}_line.json 2> $OUT/bench_$TAG.err; tail -c 400 $OUT/bench_${TAG}_line.json
python bench.py --full --workload synth512 --no-cpu-baseline --no-secondary > $OUT/bench_${TAG}_synth512.json 2>/dev/null; tail -c 300 $OUT/bench_${TAG}_synth512.json
python bench.py --mode train --steps 50 --warmup 10 > $OUT/bench_${TAG}_train.json 2>/dev/null; tail -c 300 $OUT/bench_${TAG}_train.json
python bench.py --mode train --steps 50 --warmup 10 --local-batch 2 > $OUT/bench_${TAG}_train_b2.json 2>/dev/null; tail -c 200 $OUT/bench_${TAG}_train_b2.json
python scripts/parity_report.py $OUT/parity_$TAG.json > $OUT/parity_$TAG.log 2>&1; tail -3 $OUT/parity_$TAG.log
