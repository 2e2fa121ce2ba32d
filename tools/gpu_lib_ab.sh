#!/bin/bash
# A/B of two builds of this tree (DDIM_COLD_LIB=<other .so> vs the in-tree _C.so):
# REPS (default 3) interleaved pairs of training benches (BENCH_ARGS, default
# "--steps 1000 --warmup 50"), then (unless NO_DIST=1) the 2-rank one-GPU DP check
# SAMPLER=1: the pairs run the eta = 0 DDIM sampler instead (k = 20, N = 64 graph replays,
# tools/ub_sampler_eta.py --eta0; SAMPLER_ARGS, default "64 20 5") and print ms per batch
# usage: [BENCH_ARGS=...] [REPS=n] [NO_DIST=1] [SAMPLER=1] tools/gpu_lib_ab.sh <other.so>
cd "$(dirname "$0")/.." 2>/dev/null || cd $GRAFT_REPO_ROOT
mkdir -p gpurun_out
OTHER=$1
ARGS=${BENCH_ARGS:---steps 1000 --warmup 50}
run() {
  timeout -k 10 300 env "$@" > gpurun_out/lib_ab.log 2>&1 || { tail -5 gpurun_out/lib_ab.log; exit 1; }
  echo "$1 $(grep '^{' gpurun_out/lib_ab.log | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['ms_per_step'])")"
}
run_sampler() {
  local out
  out=$(timeout -k 10 300 env "$@" 2>&1) || { echo "$out" | tail -5; exit 1; }
  echo "$1 $(echo "$out" | grep '^eta=0:')"
}
if [ "${SAMPLER:-0}" = "1" ]; then
  for rep in $(seq 1 ${REPS:-3}); do
    run_sampler X=other DDIM_COLD_LIB=$OTHER python tools/ub_sampler_eta.py ${SAMPLER_ARGS:-64 20 5} --eta0
    run_sampler X=tree python tools/ub_sampler_eta.py ${SAMPLER_ARGS:-64 20 5} --eta0
  done
  exit 0
fi
for rep in $(seq 1 ${REPS:-3}); do
  run X=other DDIM_COLD_LIB=$OTHER python bench.py $ARGS --no-sampler --no-vendor
  run X=tree python bench.py $ARGS --no-sampler --no-vendor
done
[ "${NO_DIST:-0}" = "1" ] && exit 0
timeout -k 10 300 python -u tools/dist2_gpu.py > gpurun_out/dist2.log 2>&1; rc=$?; tail -4 gpurun_out/dist2.log; exit $rc
