#!/bin/bash
# What outlives bench.py (VERDICT r04 hygiene item): processes before and after
# a bench run with the CPU baseline leg, and the plain-command N-rank rehearsal.
set -o pipefail
TAG=${1:-hyg}
cd "$GRAFT_REPO_ROOT"
RES=${RES:-bench_results}
mkdir -p $RES
ps -eo pid,ppid,pgid,sid,stat,etime,args > $RES/${TAG}_ps_before.txt
timeout -k 10 300 python3 bench.py --full --rows 1000000 --steps 4 --warmup 1 --no-full-storage > $RES/${TAG}_bench.json 2> $RES/${TAG}_bench.err || exit $?
sleep 3
ps -eo pid,ppid,pgid,sid,stat,etime,args > $RES/${TAG}_ps_after.txt
timeout -k 10 300 python3 bench.py --full --gpus 2 --host-transport --rows 2000000 --steps 4 > $RES/${TAG}_two_ranks.json 2> $RES/${TAG}_two_ranks.err || exit $?
sleep 3
ps -eo pid,ppid,pgid,sid,stat,etime,args > $RES/${TAG}_ps_after2.txt
python3 bench.py --gpus 2 > $RES/${TAG}_no_gpus.out 2>&1; echo "rc=$?" >> $RES/${TAG}_no_gpus.out
diff <(awk '{print $NF}' $RES/${TAG}_ps_before.txt | sort) <(awk '{print $NF}' $RES/${TAG}_ps_after.txt | sort); true
