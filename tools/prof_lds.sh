# LDS-pipe counters of the step kernel (separate --pmc passes, kernel trace only; B=1e5,
# one warmup + one timed step), reduced by lds_parse.py to ${OUT_DIR:-out}/lds/lds_$TAG.json:
#   [TAG=r15] [OUT_DIR=dir] [NTM_MPC_LIB=lib.so] bash tools/prof_lds.sh
# The conflict / alignment counters of the second pass are taken only where rocprofv3 -L
# lists them.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
TAG=${TAG:-r15}
OUT=$R/${OUT_DIR:-out}/lds
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
A="--steps 1 --warmup 1 --no-cpu --no-disturbed --verify 0"
timeout -k 10 300 rocprofv3 --pmc SQ_WAVES SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_WAVE_CYCLES SQ_BUSY_CU_CYCLES -d $OUT -o lds1 --output-format csv -- python3 $R/bench.py $A > $OUT/lds1.log 2>&1 || exit $?
timeout -k 10 120 rocprofv3 -L > $OUT/counters.txt 2>&1 || exit $?
P2="SQ_WAVES SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_BUSY_CYCLES"
for c in SQ_LDS_ADDR_CONFLICT SQ_LDS_UNALIGNED_STALL SQ_LDS_DATA_FIFO_FULL; do
  grep -q "$c" $OUT/counters.txt && P2="$P2 $c"
done
timeout -k 10 300 rocprofv3 --pmc $P2 -d $OUT -o lds2 --output-format csv -- python3 $R/bench.py $A > $OUT/lds2.log 2>&1 || exit $?
cd $R && python3 tools/lds_parse.py $OUT $TAG > $OUT/lds.log 2>&1 || exit $?
echo lds done
