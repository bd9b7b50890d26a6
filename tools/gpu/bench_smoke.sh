set -o pipefail
out=${1:-/tmp/pyas_bench_smoke}
mkdir -p "$out"
timeout -k 10 400 python bench.py --full > "$out/bench_default.json" 2> "$out/bench_default.err" && \
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29512 bench.py --gpus 1 --force-dist > "$out/bench_forcedist.json" 2> "$out/bench_forcedist.err"
rc=$?
timeout -k 10 60 python bench.py --gpus 2 > "$out/bench_gpus2.out" 2>&1; echo "gpus2 rc=$?" >> "$out/bench_gpus2.out"
exit $rc
