# rt_reproject_clip beside rt_reproject over the same frame (scripts/reproject_clip_ab.py): the C2 frame and the
# RTWeekend frame at 1920 x 1080 after one key step, under the library as built.  One process per frame, each under
# its own time limit; a failed step ends the script.
#   OUT     directory for the result lines (default bench_out)
# Prints one JSON line per run and a summary line per frame.
set -o pipefail
dir=${OUT:-bench_out}
mkdir -p $dir
out=$dir/reproject_clip_ab.jsonl
: > $out
for frame in c2 rtw; do
  timeout -k 10 150 python scripts/reproject_clip_ab.py --frame $frame \
    > $dir/reproject_clip_ab.one 2> $dir/reproject_clip_ab.err || { tail -20 $dir/reproject_clip_ab.err; exit 1; }
  grep '^{' $dir/reproject_clip_ab.one | tail -1 | tee -a $out
done
python - $out <<'PY'
import json, sys
for r in (json.loads(l) for l in open(sys.argv[1])):
    print(r["frame"], "rt_reproject", r["reproject_us"]["median"], "us (again", r["reproject_again_us"]["median"], "), encode",
          r["encode_us"]["median"], "us; rt_reproject_clip",
          " ".join(f"R{k} {r[f'clip_r{k}_us']['median']} us x{r['ratio_to_reproject'][f'clip_r{k}']}" for k in (1, 2, 3)),
          "; no history", r["clip_no_history_us"]["median"], "us beside rt_reproject's", r["reproject_no_history_us"]["median"],
          "us; clamped share of carried pixels", [r[f"clamped_share_r{k}"] for k in (1, 2, 3)])
PY
