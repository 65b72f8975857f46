#!/bin/bash
# GPU box: integrator parity tests, then a kernel trace of the bench (ET prelude + device integrator timing)
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=${1:-out}
mkdir -p "$O"
timeout -k 10 300 python -u -m pytest tests/test_gpu_ode.py tests/test_gpu_out.py -x -q --timeout 120 --timeout-method thread > "$O/pytest_ode.log" 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof_ode" -o run -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --profile-reps 2 > "$O/bench_ode.json" 2> "$O/bench_ode.err"
echo done
