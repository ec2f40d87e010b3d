# Same-box A/B of the refinement loop driven from the host (rt_trace_tile_work_delta, Level 2c) against the loop
# driven from the device (rt_trace_tile_counts + rt_tile_counts_step, Level 2d): scripts/tile_counts_ab.py, one
# process per side, interleaved as scripts/gpu_ab.sh does.
#   ROUNDS  interleaved repetitions (default 3); RUNS  timed runs per process (default 5)
#   OUT     directory for the result lines (default bench_out)
# Prints one JSON line per run; both sides must end on the same table and segment count (checked at the end).
set -o pipefail
dir=${OUT:-bench_out}
mkdir -p $dir
out=$dir/tile_counts_ab.jsonl
: > $out
for r in $(seq ${ROUNDS:-3}); do
  for side in host device; do
    RT_X=0 timeout -k 10 170 python scripts/tile_counts_ab.py --side $side --runs ${RUNS:-5} \
      > $dir/tile_counts_ab.one 2> $dir/tile_counts_ab.err || { tail -20 $dir/tile_counts_ab.err; exit 1; }
    grep '^{' $dir/tile_counts_ab.one | tail -1 | tee -a $out
  done
done
python - $out <<'PY'
import json, sys
rows = [json.loads(l) for l in open(sys.argv[1])]
assert len({(r["final_table_crc32"], r["segments_per_run"]) for r in rows}) == 1, "the two sides differ"
for side in ("host", "device"):
    ms = sorted(r["ms_per_round"] for r in rows if r["side"] == side)
    one = next(r for r in rows if r["side"] == side)
    print(side, "ms per round (each process's median):", ms, "host syncs per round", one["host_syncs_per_round"],
          "cull passes per run", one["cull_passes_per_run"], "resting after each round", one["tiles_resting_after_round"])
PY
