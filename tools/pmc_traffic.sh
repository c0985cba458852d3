#!/bin/bash
# One command that regenerates profiles/pmc_traffic_f32.json (and the bf16 twin) on the GPU box:
#   bash tools/pmc_traffic.sh [tag]      (raw outputs under $OUT/pmc_<tag>_<dtype>/, default OUT=scratch; every step under `timeout`)
# 1. kernel trace of the profiled command -> the kernel names the forward launches (profiles/<tag>_kernel_stats.csv)
# 2. separate --pmc passes (FETCH_SIZE | WRITE_SIZE | SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE | SQ_INSTS_VALU SQ_WAVES), as MI355X_MICROARCH.md prescribes
# 3. tools/pmc_to_json.py: per-launch HBM bytes (FETCH_SIZE x2), MFMA busy, the git commit, sha256 of the kernel sources, and a
#    check that every kernel family priced from the counters was launched by the traced command (fails otherwise)
#    (families and their sources: FAMILIES in tools/pmc_to_json.py; the f32 `attn` family counts window_attn_f32_kernel and
#    window_attn_f32_split_kernel and hashes attn_f32.hip, attn_f32_split.hip and the headers the latter includes)
# The first failing step (non-zero exit or time limit) ends the script with its status: no later pass starts on the GPU.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
TAG=${1:-r02}
OUT=${OUT:-scratch}
# pass NAME CMD..: CMD under a time limit, its output in $O/NAME.log
pass() {
  local name=$1; shift
  timeout -k 10 300 "$@" > $O/$name.log 2>&1 || { local rc=$?; echo "$DT $name failed (exit $rc)"; tail -3 $O/$name.log; exit $rc; }
}
for DT in f32 bf16; do
  O=$OUT/pmc_${TAG}_${DT}
  rm -rf $O; mkdir -p $O
  pass trace rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace -- python3 tools/profile_fwd.py $DT 3
  pass fetch rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/fetch -- python3 tools/profile_fwd.py $DT 3
  pass write rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/write -- python3 tools/profile_fwd.py $DT 3
  pass mfma rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/mfma -- python3 tools/profile_fwd.py $DT 3
  # vector-ALU instructions issued (wave-level, MFMAs included) and waves launched: the VALU-issue roof of the bf16 attention kernel
  pass valu rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES --output-format csv -d $O/valu -- python3 tools/profile_fwd.py $DT 3
  timeout -k 10 120 python3 tools/pmc_to_json.py $O $DT > $O/pmc_traffic_${DT}.json ||
    { rc=$?; echo "pmc_to_json failed for $DT (exit $rc)"; tail -3 $O/*.log; exit $rc; }
  cp $(ls $O/trace/*/*kernel_stats.csv | head -1) $O/${TAG}_fwd_${DT}_kernel_stats.csv 2>/dev/null
  head -c 1500 $O/pmc_traffic_${DT}.json
done
