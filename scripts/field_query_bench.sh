#!/bin/bash
# The field queries' measurements (scripts/field_query_bench.py; profiles/r12/field_query.md).
#   scripts/field_query_bench.sh build      the A/B builds of k_fieldlattice (no GPU): rows per strip, no column reuse
#   scripts/field_query_bench.sh run OUT    every GPU step under its own time limit, the chain ends at the first
#                                           failure; then the report (no GPU)
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
VARIANTS="r1 r4 r16 r32 nocol"
case "$1" in
build)
  for v in $VARIANTS; do
    if [ "$v" = nocol ]; then flags="-DRT_FIELD_COLUMN=0"; else flags="-DRT_FIELD_ROWS=${v#r}"; fi
    make -C gpgpuraytrace_amd/csrc variant NAME=$v FLAGS="$flags" || exit 1
  done
  python3 scripts/resource_usage.py > gpgpuraytrace_amd/_build/resource_usage.txt
  ;;
run)
  O=${2:?output directory}
  mkdir -p "$O" && rm -f "$O/field_query.jsonl"
  timeout -k 10 240 python3 scripts/field_query_bench.py run "$O" &&
  RT_LIB_VARIANT=r1 timeout -k 10 120 python3 scripts/field_query_bench.py run "$O" &&
  RT_LIB_VARIANT=r4 timeout -k 10 120 python3 scripts/field_query_bench.py run "$O" &&
  RT_LIB_VARIANT=r16 timeout -k 10 120 python3 scripts/field_query_bench.py run "$O" &&
  RT_LIB_VARIANT=r32 timeout -k 10 120 python3 scripts/field_query_bench.py run "$O" &&
  RT_LIB_VARIANT=nocol timeout -k 10 120 python3 scripts/field_query_bench.py run "$O" &&
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/kt" -o run -- \
    python3 scripts/field_query_bench.py trace > "$O/kt.log" 2>&1 &&
  python3 scripts/field_query_bench.py report "$O" --resources gpgpuraytrace_amd/_build/resource_usage.txt \
    --stats "$(find "$O/kt" -name '*kernel_stats.csv' | head -1)"
  ;;
*)
  echo "usage: $0 build | run OUT_DIR"; exit 2
  ;;
esac
