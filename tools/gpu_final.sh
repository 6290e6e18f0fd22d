# Final-tree numbers: bench at the driver's settings and the config sweep.
set -o pipefail
TAG=${1:-final}
cd "$GRAFT_REPO_ROOT"
RES=${RES:-bench_results}
mkdir -p $RES
timeout -k 10 400 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $RES/${TAG}_bench.json 2> $RES/${TAG}_bench.err || { tail -20 $RES/${TAG}_bench.err; exit 1; }
cut -c1-400 $RES/${TAG}_bench.json
timeout -k 10 400 python3 tools/bench_configs.py > $RES/${TAG}_configs.json 2> $RES/${TAG}_configs.err || { tail -20 $RES/${TAG}_configs.err; exit 1; }
echo configs done
