# rt_reproject's time beside rt_encode_rgba8 over the same frame (scripts/reproject_ab.py): the C2 frame and the
# RTWeekend frame at 1920 x 1080 after one key step, under the library as built.  One process per frame, each under
# its own time limit; a failed step ends the script.
#   OUT     directory for the result lines (default bench_out)
# Prints one JSON line per run and a summary line per frame.
set -o pipefail
dir=${OUT:-bench_out}
mkdir -p $dir
out=$dir/reproject_ab.jsonl
: > $out
for frame in c2 rtw; do
  timeout -k 10 150 python scripts/reproject_ab.py --frame $frame \
    > $dir/reproject_ab.one 2> $dir/reproject_ab.err || { tail -20 $dir/reproject_ab.err; exit 1; }
  grep '^{' $dir/reproject_ab.one | tail -1 | tee -a $out
done
python - $out <<'PY'
import json, sys
for r in (json.loads(l) for l in open(sys.argv[1])):
    print(r["frame"], "encode", r["encode_us"]["median"], "us; reproject", r["reproject_us"]["median"], "us, with Rgba8",
          r["reproject_rgba8_us"]["median"], "us, no history", r["no_history_us"]["median"], "us; streaming rate gives",
          r["streaming_us"], "us; over streaming", r["over_streaming"], "; carried", r["carried_pixels"], "of",
          r["hit_pixels"], "hit pixels")
PY
