#!/bin/bash
# tools/arena_table_vs_parent.py under the shipped library and under a build of the parent commit, a fresh process and a time
# limit per run; the first run that fails ends the script.
#   tools/arena_table_vs_parent.sh PARENT_LIB.so OUT_DIR
# OUT_DIR/outputs_vs_parent.txt: the hash lines and whether the parent's are the same; OUT_DIR/time_vs_parent.json: the timed
# launches (the two libraries in alternating processes) and tools/server_opt_time.py's, judged against the parent's own spread.
set -u -o pipefail
PARENT=$(realpath "$1"); OUT=$2
cd "$(dirname "$0")/.." && mkdir -p "$OUT"
NEW=$(realpath fedmlp_amd/libfedmlp_hip.so)
FEDMLP_HIP_LIB=$NEW timeout -k 10 300 python tools/arena_table_vs_parent.py > "$OUT/outputs_new.txt" || exit $?
FEDMLP_HIP_LIB=$PARENT timeout -k 10 300 python tools/arena_table_vs_parent.py > "$OUT/outputs_parent.txt" || exit $?
{ cat "$OUT/outputs_new.txt"
  if diff "$OUT/outputs_parent.txt" "$OUT/outputs_new.txt"; then echo "parent build: the same $(wc -l < "$OUT/outputs_new.txt") lines"
  else echo "parent build: DIFFERS (lines above: < parent, > this tree)"; fi; } > "$OUT/outputs_vs_parent.txt"
tail -n 1 "$OUT/outputs_vs_parent.txt"
: > "$OUT/time_lines.jsonl"
for round in 1 2; do
    for lib in "$PARENT" "$NEW"; do
        FEDMLP_HIP_LIB=$lib timeout -k 10 300 python tools/arena_table_vs_parent.py --time >> "$OUT/time_lines.jsonl" || exit $?
    done
done
FEDMLP_HIP_LIB=$PARENT timeout -k 10 300 python tools/server_opt_time.py --out "$OUT/server_parent.json" > /dev/null || exit $?
FEDMLP_HIP_LIB=$NEW timeout -k 10 300 python tools/server_opt_time.py --out "$OUT/server_new.json" > /dev/null || exit $?
python tools/arena_table_vs_parent.py --judge "$OUT/time_lines.jsonl" "$OUT/server_parent.json" "$OUT/server_new.json" "$OUT/time_vs_parent.json"
