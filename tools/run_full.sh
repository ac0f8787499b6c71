#!/bin/bash
# full GPU validation: the whole -m gpu suite (log written directly: no pipe), smoke, the whole bench line (bench.py --full);
# stops at the first step that does not exit 0
#   tools/run_full.sh <tag> <output dir>
cd "$(dirname "$0")/.."
tag=${1:?usage: tools/run_full.sh <tag> <output dir>}
out=${2:?usage: tools/run_full.sh <tag> <output dir>}
mkdir -p "$out"
timeout -k 10 1000 python -m pytest tests -m gpu -q --tb=short > "$out/${tag}_tests.log" 2>&1; rc=$?
echo "tests rc=$rc" | tee -a "$out/${tag}_tests.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$out/${tag}_smoke.log" 2>&1; rc=$?
echo "smoke rc=$rc"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err"; rc=$?
echo "bench rc=$rc"; exit $rc
