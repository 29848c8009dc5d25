# headline throughput under four pipeline configurations; logs go to the directory given as $1
set -e
O="${1:-bench_out}"
mkdir -p "$O"
python bench.py --steps 30 > "$O/b1.log" 2>&1
python bench.py --steps 30 --no-numa > "$O/b2.log" 2>&1
python bench.py --steps 30 --micro-batch 131072 > "$O/b3.log" 2>&1
python bench.py --steps 30 --micro-batch 524288 --pipeline-depth 3 > "$O/b4.log" 2>&1
python scripts/probe_pipe.py > "$O/probe3.log" 2>&1
for f in "$O"/b*.log; do echo $f; grep -o '"value": [0-9.]*\|ms_per_step": [0-9.]*\|numa_node": [0-9a-z]*\|host_submit_ms_per_step": [0-9.]*' $f; done
