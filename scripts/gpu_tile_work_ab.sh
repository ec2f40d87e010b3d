# Same-box A/B of one rt_trace_tile_work call per round against four rt_trace_tiles calls per round
# (scripts/tile_work_ab.py; one process per side, interleaved as scripts/gpu_ab.sh does).
#   ROUNDS  interleaved repetitions (default 3); STEPS / WARMUP  timed / warm-up rounds per process (8 / 6)
#   OUT     directory for the result lines (default bench_out)
# Prints one JSON line per run; the two sides' segments per round must be equal (checked at the end).
set -o pipefail
dir=${OUT:-bench_out}
mkdir -p $dir
out=$dir/tile_work_ab.jsonl
: > $out
for r in $(seq ${ROUNDS:-3}); do
  for side in work tiles; do
    RT_X=0 timeout -k 10 170 python scripts/tile_work_ab.py --side $side --rounds ${STEPS:-8} --warmup ${WARMUP:-6} \
      > $dir/tile_work_ab.one 2> $dir/tile_work_ab.err || { tail -20 $dir/tile_work_ab.err; exit 1; }
    grep '^{' $dir/tile_work_ab.one | tail -1 | tee -a $out
  done
done
python - $out <<'PY'
import json, sys
rows = [json.loads(l) for l in open(sys.argv[1])]
segs = {r["segments_per_round"] for r in rows}
assert len(segs) == 1, segs
for side in ("work", "tiles"):
    ms = sorted(r["ms_per_round"] for r in rows if r["side"] == side)
    print(side, "ms per round (each process's median):", ms, "segments per round", next(iter(segs)))
PY
