#!/bin/bash
# one gpurun call at the end of a round: the whole -m gpu suite, then the committed bench lines
#   OUT=<log directory> scripts/gpu_round_final.sh <tag>  ->  $OUT/<tag>_{pytest.log,bench.json,bench_f513.jsonl,dropin.jsonl,smoke.log}
set -o pipefail
TAG=${1:-r05}
OUT=${OUT:?usage: OUT=<log directory> scripts/gpu_round_final.sh <tag> [notests]}
mkdir -p "$OUT"
if [ "${2:-tests}" != "notests" ]; then
timeout -k 10 1000 python -X faulthandler -m pytest tests -m gpu -x -q --durations=8 -o faulthandler_timeout=400 > $OUT/${TAG}_pytest.log 2>&1
rc=$?; tail -6 $OUT/${TAG}_pytest.log; [ $rc -ne 0 ] && exit $rc
fi
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 || { tail -20 $OUT/${TAG}_smoke.log; exit 1; }
echo "== bench.py"
timeout -k 10 400 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { tail -20 $OUT/${TAG}_bench.err; exit 1; }
tail -c 1500 $OUT/${TAG}_bench.json
echo "== bench_f513"
timeout -k 10 400 python scripts/bench_f513.py a11 c4h c4w c5 mel melh melw smallr tw20 tw30h im50 > $OUT/${TAG}_bench_f513.jsonl 2> $OUT/${TAG}_bench_f513.err || { tail -20 $OUT/${TAG}_bench_f513.err; exit 1; }
cut -c 1-420 $OUT/${TAG}_bench_f513.jsonl
echo "== bench_dropin"
timeout -k 10 900 python scripts/bench_dropin.py pcie a11 c2 c4 mel c4mel c4m > $OUT/${TAG}_dropin.jsonl 2> $OUT/${TAG}_dropin.err || { tail -20 $OUT/${TAG}_dropin.err; exit 1; }
cut -c 1-500 $OUT/${TAG}_dropin.jsonl
echo "== bench_online"
timeout -k 10 300 python scripts/bench_online.py > $OUT/${TAG}_bench_online.jsonl 2> $OUT/${TAG}_bench_online.err || { tail -20 $OUT/${TAG}_bench_online.err; exit 1; }
cut -c 1-400 $OUT/${TAG}_bench_online.jsonl
