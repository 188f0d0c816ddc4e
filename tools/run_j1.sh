set -e -o pipefail
O=${O:-bench_out}; mkdir -p "$O"
timeout -k 10 300 python3 -u -c "import __graft_entry__ as g; g.smoke()" > $O/fin_smoke.log 2>&1
tail -2 $O/fin_smoke.log
timeout -k 10 900 python3 -u -m pytest -x -q --timeout 120 --timeout-method thread tests -m gpu > $O/fin_gpu.log 2>&1
tail -2 $O/fin_gpu.log
timeout -k 10 300 python3 -u bench.py --full > $O/fin_bench.log 2>&1
tail -1 $O/fin_bench.log
