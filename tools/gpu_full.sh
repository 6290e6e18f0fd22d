# Full GPU suite + bench at the driver's settings, each step under its own limit.
set -o pipefail
TAG=${1:-full}
cd "$GRAFT_REPO_ROOT"
RES=${RES:-bench_results}
mkdir -p $RES
timeout -k 10 900 python -u -m pytest -x -q --timeout 240 --timeout-method thread -m gpu tests > $RES/${TAG}_gputests.log 2>&1 || { tail -30 $RES/${TAG}_gputests.log; exit 1; }
tail -2 $RES/${TAG}_gputests.log
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $RES/${TAG}_smoke.log 2>&1 || { tail -20 $RES/${TAG}_smoke.log; exit 1; }
timeout -k 10 400 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $RES/${TAG}_bench.json 2> $RES/${TAG}_bench.err || { tail -20 $RES/${TAG}_bench.err; exit 1; }
cat $RES/${TAG}_bench.json
