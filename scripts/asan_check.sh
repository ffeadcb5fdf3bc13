#!/bin/bash
# Host-ASan build of libpdd + the C-ABI driver tests/native/abi_asan.cpp
# (host code instrumented; device code built normally for gfx950).  Build
# here, run on the GPU box:  scripts/asan_check.sh build | run
# plan: the sweep planner alone (tests/native/plan_dump.cpp, plain C++ with
# -fsanitize=address,undefined) over every case of
# tests/golden/golden_sweep_plans.json, on the CPU.
# Sources: pypulsar_amd/_digest.py, the production build's own list.
set -e
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
case "${1:-build}" in
  build)
    mkdir -p build
    SRCS=$(python3 -c "from pypulsar_amd import _digest as d; print(' '.join('pypulsar_amd/csrc/' + s for s in d.SOURCES))")
    /opt/rocm/bin/hipcc -O3 -g --offload-arch=gfx950 -std=c++17 -fno-slp-vectorize -ffp-contract=off \
      -Xarch_host -fsanitize=address -Xarch_host -fno-omit-frame-pointer \
      -Iinclude -Ipypulsar_amd/csrc -o build/abi_asan tests/native/abi_asan.cpp $SRCS
    ;;
  run)
    set +e
    mkdir -p gpurun_out
    ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 timeout -k 10 300 ./build/abi_asan > gpurun_out/abi_asan.log 2>&1
    rc=$?; tail -20 gpurun_out/abi_asan.log; exit $rc
    ;;
  plan)
    mkdir -p build
    CXX=$(command -v c++ || echo /opt/rocm/lib/llvm/bin/clang++)
    $CXX -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
      -fno-omit-frame-pointer -ffp-contract=off -Ipypulsar_amd/csrc -o build/plan_dump_asan \
      tests/native/plan_dump.cpp pypulsar_amd/csrc/pdd_sweep_plan.hip
    python3 - <<'EOF'
import sys
sys.path[:0] = ["tests", "."]
import test_sweep_plan as t
for c in t.CASES:
    got = t.run_plan(t.case_table(c), c["dtype"], c["flags"], "build/plan_dump_asan")
    assert got == c["want"], c["name"]
print("plan_dump under ASan + UBSan: %d cases clean and equal to the golden plans" % len(t.CASES))
EOF
    ;;
esac
