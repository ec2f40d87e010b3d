# rt_denoise's time per pass beside rt_encode_rgba8 over the same frame (scripts/denoise_ab.py): the C2 frame and the
# RTWeekend frame at 1920 x 1080, under the library as built and under the two builds that force one kernel shape,
#   make -C simd-ray-tracer_amd variant NAME=dn_direct KFLAGS=-DRTK_DENOISE_SHAPE=0
#   make -C simd-ray-tracer_amd variant NAME=dn_lds    KFLAGS=-DRTK_DENOISE_SHAPE=1
# (built beforehand; a build that is missing is left out).  One process per frame and build, each under its own time
# limit; a failed step ends the script.
#   OUT     directory for the result lines (default bench_out)
# Prints one JSON line per run; every build of a frame must give the same Out and Rgba8 (checked at the end).
set -o pipefail
dir=${OUT:-bench_out}
mkdir -p $dir
out=$dir/denoise_ab.jsonl
: > $out
for frame in c2 rtw; do
  for lib in librt_trace.so librt_trace_dn_direct.so librt_trace_dn_lds.so; do
    [ -f simd-ray-tracer_amd/$lib ] || continue
    RT_TRACE_LIB=$lib timeout -k 10 150 python scripts/denoise_ab.py --frame $frame \
      > $dir/denoise_ab.one 2> $dir/denoise_ab.err || { tail -20 $dir/denoise_ab.err; exit 1; }
    grep '^{' $dir/denoise_ab.one | tail -1 | tee -a $out
  done
done
python - $out <<'PY'
import json, sys
rows = [json.loads(l) for l in open(sys.argv[1])]
for frame in ("c2", "rtw"):
    mine = [r for r in rows if r["frame"] == frame]
    assert len({(r["out_crc32"], r["rgba8_crc32"]) for r in mine}) == 1, f"{frame}: the builds differ"
    for r in mine:
        print(frame, r["lib"], "encode", r["encode_us"]["median"], "us; passes", r["pass_us"], "us; over streaming",
              r["pass_over_streaming"], "; default total", r["total_us"][str(r["defaults"]["iterations"])]["median"],
              "with Rgba8", r["total_rgba8_us"]["median"], "; first hit", r["first_hit_us"]["median"])
PY
