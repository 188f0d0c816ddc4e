#!/bin/bash
# Round-6: the whole GPU suite (new DDP / parity / LN-fold tests included), then the default
# bench line.  Each step has its own limit.
cd "$(dirname "$0")/.."; O=${O:-$(pwd)/bench_out}; mkdir -p "$O"
TAG=${TAG:-r6h}
timeout -k 10 1000 python3 -u -m pytest tests -m gpu -q --timeout 300 --timeout-method thread \
  -p no:cacheprovider > $O/${TAG}_gpu_tests.log 2>&1
rc=$?; echo "gpu tests rc=$rc"; tail -3 $O/${TAG}_gpu_tests.log
grep -E "^FAILED|^ERROR" $O/${TAG}_gpu_tests.log | head -20
case $rc in 124|134|137|139) exit $rc;; esac
timeout -k 10 300 python3 bench.py --full > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err
rc2=$?; echo "bench rc=$rc2"; cat $O/${TAG}_bench.json | cut -c1-600
exit $rc
