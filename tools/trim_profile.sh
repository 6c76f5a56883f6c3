#!/bin/bash
# Profile of the fp16mx forward for one value of a tuning option (default 9, SPEF_OPT_TRIM; run on a machine with the GPU):
#   bash tools/trim_profile.sh <tag> <value> <outdir> [option id]
#   <outdir>/<tag>/prof/      rocprofv3 --kernel-trace --stats of the headline workload (bench.py, 10 steps + the leg)
#   <outdir>/<tag>/pmc_<n>/   counter passes over tools/fwd_only.py, one rocprofv3 run per set and counters only:
#                               FETCH_SIZE, WRITE_SIZE, the L2 request / hit counters, the two SQ sets of tools/pmc.sh
# then: python tools/rocprof_summary.py --tag <tag> --stats <outdir>/<tag>/prof --fetch <outdir>/<tag>/pmc_1 \
#         --write <outdir>/<tag>/pmc_2 --leg 10 --per-step front_mx_kernel
#       python tools/pmc_table.py <outdir>/<tag> > profiles/<tag>_pmc_counters.txt
set -e
TAG=$1; VAL=$2; OUT=${3:?usage: trim_profile.sh <tag> <value> <outdir> [option id]}; OPT=${4:-9}
export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/.." && pwd)
case $OUT in /*) O=$OUT/$TAG ;; *) O=$R/$OUT/$TAG ;; esac
mkdir -p $O
(cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof -o run --output-format csv \
  -- python3 $R/bench.py --gpus 1 --steps 10 --full --set-option $OPT=$VAL --no-cpu-baseline --no-int8 --no-keypoint --no-x2 \
     --no-fp16 --sharp-frames 0 --no-peaks --detail-out '') > $O/prof.log 2>&1
echo "stats ok"
i=0
for set in "FETCH_SIZE" "WRITE_SIZE" "TCP_TCC_READ_REQ_sum TCC_REQ_sum TCC_HIT_sum TCC_MISS_sum" \
           "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS" \
           "SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_MFMA SQ_INSTS_VMEM_RD SQ_INSTS_SALU SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES"; do
  i=$((i+1))
  (cd /tmp && DT=fp16mx OPTS="$OPT=$VAL" timeout -s KILL 150 rocprofv3 --pmc $set -d $O/pmc_$i -o run --output-format csv \
    -- python3 $R/tools/fwd_only.py 2) > $O/pmc_$i.log 2>&1
  echo "pass $i ok"
done
