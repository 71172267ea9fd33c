#!/bin/bash
# GPU-box run: smoke, full parity suite, N=1 bench with every part (each step time-limited; stop at the first failure).
# Logs go to $OUT_DIR (default: out/ under the repository root).
set -o pipefail
cd "$GRAFT_REPO_ROOT"
O=${OUT_DIR:-out}
mkdir -p "$O"
export NCCL_AMD_SPIN_TIMEOUT_MS=20000
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1 && echo SMOKE_OK &&
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 240 --timeout-method thread > "$O/pytest_gpu.log" 2>&1 && echo PYTEST_OK &&
timeout -k 10 300 python -u bench.py --full ${BENCH_ARGS} > "$O/bench1.log" 2>&1 && echo BENCH_OK
tail -3 "$O/pytest_gpu.log"; tail -c 3000 "$O/bench1.log"
