#!/bin/bash
# One GPU-box session: parity tests -> smoke -> bench -> rocprof kernel trace.
# Every GPU step has its own time limit; steps chained with && (stop at first failure).
set -o pipefail
cd "$(dirname "$0")/.."
OUT="${FA_OUT:-bench_out}"
mkdir -p "$OUT"
export TMPDIR=/tmp
STEPS="${1:-all}"
run_tests() { timeout -k 10 ${T_TESTS:-900} python -u -m pytest tests -x -v -m gpu --timeout 300 --timeout-method thread ${PYTEST_ARGS:-} > "$OUT"/pytest_gpu.log 2>&1; }
run_smoke() { timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT"/smoke.log 2>&1; }
run_bench() { timeout -k 10 600 python bench.py --full ${BENCH_ARGS:---steps 20 --warmup 5} > "$OUT"/bench.log 2>&1; }
run_prof()  { timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/prof -o fwd -- python3 bench.py --full --no-cpu ${PROF_ARGS:-} > "$OUT"/prof.log 2>&1; }
case "$STEPS" in
  all)   run_tests && run_smoke && run_bench && run_prof ;;
  tests) run_tests ;;
  bench) run_bench ;;
  prof)  run_prof ;;
  smoke) run_smoke ;;
  *)     eval "$STEPS" ;;
esac
rc=$?
echo "exit $rc"
for f in "$OUT"/*.log; do echo "== $f"; tail -n 5 "$f"; done
exit $rc
