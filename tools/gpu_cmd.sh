set -o pipefail
mkdir -p ${OUT_DIR:-out}
timeout -k 10 600 python -u -m pytest tests/ -q -m gpu -p no:cacheprovider -x --timeout 300 --timeout-method thread > ${OUT_DIR:-out}/parity.log 2>&1
rc=$?; echo "pytest rc=$rc" >> ${OUT_DIR:-out}/parity.log
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 300 python tools/diag_phases.py 100000 > ${OUT_DIR:-out}/phases.log 2>&1 || exit $?
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 --no-cpu > ${OUT_DIR:-out}/bench.json 2> ${OUT_DIR:-out}/bench.err || exit $?
