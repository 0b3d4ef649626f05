# A/B timing of two builds of the library on one box (alternating, ROUNDS rounds,
# default 2):
#   [ROUNDS=3] [AB_TAG=c3] [OUT_DIR=dir] bash tools/ab_bench.sh <libA.so> <libB.so> [bench args...]
# Prints ms_per_step of each run; results in ${OUT_DIR:-out}/ab_[<tag>_]*.json.
set -o pipefail
D=${OUT_DIR:-out}
mkdir -p $D
A=$1; B=$2; shift 2
T=${AB_TAG:+${AB_TAG}_}
for r in $(seq 1 ${ROUNDS:-2}); do
  for v in A B; do
    lib=$A; [ $v = B ] && lib=$B
    NTM_MPC_LIB=$lib timeout -k 10 200 python bench.py --no-cpu "$@" > $D/ab_${T}${v}_$r.json 2>/dev/null || exit 1
    python -c "import json,sys; d=json.load(open('$D/ab_${T}${v}_$r.json')); print('$v', $r, round(d['ms_per_step'], 3))"
  done
done
