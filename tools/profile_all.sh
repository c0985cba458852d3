#!/bin/bash
# Everything the round commits under profiles/, regenerated on the GPU box in ONE gpurun call (every rocprofv3 pass under `timeout`,
# counters in their own passes):   bash tools/profile_all.sh r04
#   tools/profile_round.sh  -> forward kernel stats + PMC traffic JSONs, training kernel stats, training PMC table + pmc_train.json,
#                              kernel micro-benchmarks, the full bench line (raw outputs under $OUT, default scratch)
#   tools/pmc_per_shape.py  -> per-shape clock / MFMA-busy of the forward kernels
#   tools/pmc_issue_table.sh (forward bf16, training bf16, training f32) -> issuing / stalled / parked, LDS busy + conflicts, MFMA busy
#   tools/per_step_kernels.sh (bf16, f32) -> exact per-step kernel lists of the training step
#   1-rank RCCL run of the bench's training section (PANGU_DIST_FORCE=1, bench.py --full -> profiles/<tag>_rccl_1rank.json)
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
TAG=${1:-r04}
export OUT=${OUT:-scratch}      # raw outputs of this script and of tools/profile_round.sh
mkdir -p $OUT
bash tools/profile_round.sh $TAG > $OUT/${TAG}_round.log 2>&1
for DT in f32 bf16; do
  python3 tools/pmc_per_shape.py $OUT/pmc_${TAG}_${DT}/mfma > $OUT/${TAG}_fwd_${DT}_per_shape.md 2>> $OUT/${TAG}_round.log
done
bash tools/pmc_issue_table.sh > $OUT/${TAG}_fwd_bf16_issue_table.md 2>> $OUT/${TAG}_round.log
bash tools/pmc_issue_table.sh train bf16 > $OUT/${TAG}_train_bf16_issue_table.md 2>> $OUT/${TAG}_round.log
bash tools/pmc_issue_table.sh train f32 > $OUT/${TAG}_train_f32_issue_table.md 2>> $OUT/${TAG}_round.log
bash tools/per_step_kernels.sh bf16 > $OUT/${TAG}_train_bf16_per_step.md 2>> $OUT/${TAG}_round.log
bash tools/per_step_kernels.sh f32 > $OUT/${TAG}_train_f32_per_step.md 2>> $OUT/${TAG}_round.log
RANK=0 WORLD_SIZE=1 LOCAL_RANK=0 MASTER_ADDR=127.0.0.1 MASTER_PORT=29531 PANGU_DIST_FORCE=1 timeout 600 python3 bench.py --full --no-bf16 --cpu-baseline none --steps 3 --warmup 1 > profiles/${TAG}_rccl_1rank.json
ls -la $OUT/${TAG}_* | head -40
