#!/bin/bash
# Regenerates the round's committed measurements on the GPU box (every step under `timeout`, and the first
# failing step -- non-zero exit or time limit -- ends the script with its status: no later step starts on the GPU):
#   bash tools/profile_round.sh r02
# -> $OUT/<tag>_* (default OUT=scratch): forward kernel stats + PMC traffic JSONs (tools/pmc_traffic.sh), training-step kernel stats per dtype,
#    the training PMC table (FETCH_SIZE | WRITE_SIZE | MFMA busy, three separate passes), the kernel micro-benchmarks and the
#    full bench line (bench.py --full, written to profiles/<tag>_bench.json).  Copy what else is to be judged into profiles/.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
TAG=${1:-r02}
export OUT=${OUT:-scratch}      # raw outputs; tools/pmc_traffic.sh writes there too
fail() { echo "profile_round.sh: $1 failed (exit $2)" >&2; exit $2; }
mkdir -p $OUT
timeout -k 10 3600 bash tools/pmc_traffic.sh $TAG > $OUT/${TAG}_pmc_traffic.log 2>&1 || fail "tools/pmc_traffic.sh" $?
# bench.py reads roofline.traffic from profiles/pmc_traffic_<dtype>.json (and checks the kernel sources' hashes): let the
# bench line at the end of this script see the tables just measured
cp $OUT/pmc_${TAG}_f32/pmc_traffic_f32.json $OUT/pmc_${TAG}_bf16/pmc_traffic_bf16.json profiles/ 2>/dev/null
for DT in f32 bf16; do
  rm -rf /tmp/tr_$DT
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/tr_$DT -- python3 tools/profile_train.py $DT 3 1 > $OUT/${TAG}_train_${DT}.log 2>&1 || fail "$DT training trace" $?
  cp "$(find /tmp/tr_$DT -name '*kernel_stats.csv' | head -1)" $OUT/${TAG}_train_${DT}_kernel_stats.csv
done
# per dtype (the two steps share kernel names -- Adam, row kernels, the reduce launch -- so each gets its own passes): per-kernel
# table + whole-step byte totals (profiles/pmc_train.json: bench.py's training roofline blocks)
for DT in f32 bf16; do
  P=/tmp/trpmc_$DT; rm -rf $P; mkdir -p $P
  timeout -k 10 400 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $P/p1 -- python3 tools/profile_train.py $DT 2 1 > $P/p1.log 2>&1 || fail "$DT FETCH_SIZE pass" $?
  timeout -k 10 400 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $P/p2 -- python3 tools/profile_train.py $DT 2 1 > $P/p2.log 2>&1 || fail "$DT WRITE_SIZE pass" $?
  timeout -k 10 400 rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $P/p3 -- python3 tools/profile_train.py $DT 2 1 > $P/p3.log 2>&1 || fail "$DT MFMA pass" $?
  echo "## $DT training step" >> $OUT/${TAG}_train_pmc_table.md
  timeout -k 10 120 python3 tools/pmc_train_table.py $P >> $OUT/${TAG}_train_pmc_table.md 2>> $OUT/${TAG}_train_pmc_table.err || fail "$DT pmc_train_table.py" $?
  # the same command with ZERO measured steps (model construction + init + the warm-up step): subtracted from the byte totals
  mkdir -p ${P}_w0
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d ${P}_w0/p1 -- python3 tools/profile_train.py $DT 0 1 > ${P}_w0/p1.log 2>&1 || fail "$DT warm-up FETCH_SIZE pass" $?
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d ${P}_w0/p2 -- python3 tools/profile_train.py $DT 0 1 > ${P}_w0/p2.log 2>&1 || fail "$DT warm-up WRITE_SIZE pass" $?
done
timeout -k 10 120 python3 tools/pmc_train_table.py --json $OUT/pmc_train.json /tmp/trpmc_f32 /tmp/trpmc_bf16 2 || fail "pmc_train_table.py --json" $?
cp $OUT/pmc_train.json profiles/
{
  for sec in mlp_fused mlp_train attn_qkv_bf16 attn_bf16 gemm_bf16 wgrad_bf16 gemm_ln_bf16 attn attn_bwd gemm wgrad; do
    echo "## $sec"
    timeout -k 10 400 python3 tools/bench_kernels.py $sec --lib-compare 2>&1 | grep -v "amdgpu.ids"
    rc=${PIPESTATUS[0]}; [ $rc -eq 0 ] || fail "bench_kernels.py $sec" $rc
  done
} > $OUT/${TAG}_kernel_microbench.txt
timeout -k 10 900 python3 bench.py --full > profiles/${TAG}_bench.json || fail "bench.py --full" $?
tail -c 600 profiles/${TAG}_bench.json
