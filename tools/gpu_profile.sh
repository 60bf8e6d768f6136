# rocprofv3 kernel-trace + stats of a short bench run (ROCm 7.2).
set -o pipefail
cd $GRAFT_REPO_ROOT
mkdir -p gpurun_out
export TMPDIR=/tmp
OUT=${1:-prof}
bash tools/gpu_run.sh $OUT "prof:--full --steps 5 --warmup 2 --no-cpu-baseline"
echo "PROF EXIT $?"
find gpurun_out/$OUT -name "*stats*" | head
