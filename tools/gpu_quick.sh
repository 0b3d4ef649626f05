# Parity suite (every -m gpu test) + the default bench; each GPU step has its own limit.
set -o pipefail
mkdir -p ${OUT_DIR:-out}
timeout -k 10 700 python -u -m pytest tests -q -m gpu -p no:cacheprovider --timeout 240 --timeout-method thread -rf > ${OUT_DIR:-out}/parity.log 2>&1
rc=$?
tail -15 ${OUT_DIR:-out}/parity.log
[ $rc -eq 0 ] || [ $rc -eq 1 ] || exit $rc
timeout -k 10 400 python bench.py --full ${BENCH_ARGS:-} > ${OUT_DIR:-out}/bench.json 2> ${OUT_DIR:-out}/bench.err || exit $?
cat ${OUT_DIR:-out}/bench.json
