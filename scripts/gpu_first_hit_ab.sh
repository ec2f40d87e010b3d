# rt_trace_first_hit's time beside the one-frame, one-bounce trace launch of the same frame (scripts/first_hit_ab.py):
# the C2 frame and the RTWeekend frame at 1920 x 1080; all three planes, Hit alone, Cull off, and the yardstick.
# One process per variant, each under its own time limit; a failed step ends the script.
#   OUT     directory for the result lines (default bench_out)
# Prints one JSON line per variant; the three first-hit variants of a frame must agree on the Key plane (checked at the end).
set -o pipefail
dir=${OUT:-bench_out}
mkdir -p $dir
out=$dir/first_hit_ab.jsonl
: > $out
for frame in c2 rtw; do
  for variant in all hit cull_off trace; do
    timeout -k 10 120 python scripts/first_hit_ab.py --frame $frame --variant $variant \
      > $dir/first_hit_ab.one 2> $dir/first_hit_ab.err || { tail -20 $dir/first_hit_ab.err; exit 1; }
    grep '^{' $dir/first_hit_ab.one | tail -1 | tee -a $out
  done
done
python - $out <<'PY'
import json, sys
rows = [json.loads(l) for l in open(sys.argv[1])]
for frame in ("c2", "rtw"):
    keys = {(r["key_crc32"], r["hit_pixels"]) for r in rows if r["frame"] == frame and r["variant"] != "trace"}
    assert len(keys) == 1, f"{frame}: the first-hit variants differ"
    for r in rows:
        if r["frame"] == frame:
            print(frame, r["variant"], "us median", r["us_median"], "range", r["us_min"], "-", r["us_max"])
PY
