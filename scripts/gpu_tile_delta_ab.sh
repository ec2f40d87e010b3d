# Same-box A/B/C of the per-tile change statistics (scripts/tile_delta_ab.py; one process per side,
# interleaved as scripts/gpu_tile_work_ab.sh does):
#   base   the parent commit's library (bash scripts/build_base_lib.sh HEAD base, built beforehand)
#          running rt_trace_tile_work
#   plain  this library running rt_trace_tile_work
#   delta  this library running rt_trace_tile_work_delta
#   ROUNDS  interleaved repetitions (default 3); STEPS / WARMUP  timed / warm-up rounds per process (8 / 6)
#   OUT     directory for the result lines (default bench_out)
# Every GPU step runs under its own timeout and the script stops at the first failure.  Prints one JSON
# line per run and each side's medians; the sides' segments per round must be equal (checked at the end).
set -o pipefail
dir=${OUT:-bench_out}
mkdir -p $dir
out=$dir/tile_delta_ab.jsonl
: > $out
[ -f simd-ray-tracer_amd/librt_trace_base.so ] || { echo "librt_trace_base.so is missing: bash scripts/build_base_lib.sh HEAD base" >&2; exit 1; }
orders=("base plain delta" "plain delta base" "delta base plain")  # (no side always runs first)
for r in $(seq ${ROUNDS:-3}); do
  for side in ${orders[$((r % 3))]}; do
    if [ $side = base ]; then lib=librt_trace_base.so; s=plain; else lib=librt_trace.so; s=$side; fi
    RT_TRACE_LIB=$lib timeout -k 10 170 python scripts/tile_delta_ab.py --side $s --rounds ${STEPS:-8} --warmup ${WARMUP:-6} \
      > $dir/tile_delta_ab.one 2> $dir/tile_delta_ab.err || { tail -20 $dir/tile_delta_ab.err; exit 1; }
    grep '^{' $dir/tile_delta_ab.one | tail -1 | tee -a $out
  done
done
python - $out <<'PY'
import json, sys
rows = [json.loads(l) for l in open(sys.argv[1])]
segs = {r["segments_per_round"] for r in rows}
assert len(segs) == 1, segs
for name, lib, side in (("base  rt_trace_tile_work      ", "librt_trace_base.so", "plain"),
                        ("this  rt_trace_tile_work      ", "librt_trace.so", "plain"),
                        ("this  rt_trace_tile_work_delta", "librt_trace.so", "delta")):
    ms = sorted(r["ms_per_round"] for r in rows if r["lib"] == lib and r["side"] == side)
    print(name, "ms per round (each process's median):", ms, "segments per round", next(iter(segs)))
PY
