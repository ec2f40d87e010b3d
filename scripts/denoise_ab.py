"""HIP-event time of rt_denoise on one 1920 x 1080 frame beside the box's plain streaming pass (DESIGN.md §3,
"The filter over the first-hit planes"): one frame and one library build per process.

  --frame c2 | rtw     scene 1 prefix 64 (the C2 frame) or scene 2 (RTWeekend), the scene's default camera
  RT_TRACE_LIB         the library build: librt_trace.so routes each pass to a kernel shape by its step; the builds
                       make -C simd-ray-tracer_amd variant NAME=dn_direct KFLAGS=-DRTK_DENOISE_SHAPE=0 and
                       NAME=dn_lds KFLAGS=-DRTK_DENOISE_SHAPE=1 force one shape for every step

The input is the 1-spp running mean of rt_trace (8 bounces) and rt_trace_first_hit's three planes of frame 0.  Under
the library's defaults for NormalPower and the sigmas the script times, each as 30 calls after 5 warm-ups between two
HIP events on one stream, median and range in microseconds:
  total[n]      rt_denoise with Iterations = n for n = 1 .. 5, no Rgba8; pass[i] = total[i + 1] - total[i] is the
                pass at step 2^i (the medians' difference: every pass of a call does the same work whatever it reads)
  total_rgba8   the default Iterations with Rgba8
  encode        rt_encode_rgba8 over the same frame: 16 B read and 4 B written per pixel, the plain streaming pass;
                its rate prices each pass's algorithmic bytes -- colour in and out (16 + 16), Hit (8) and, with the
                normal stop, Normal (16), once each per pixel -- and ratio[i] = pass[i] / (those bytes / that rate)
  first_hit     rt_trace_first_hit's three planes, for scale
and prints one JSON line, with a checksum of Out at the default Iterations (the same for every build)."""
import argparse
import json
import os
import pathlib
import statistics
import sys
import zlib

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

W, H, CALLS, WARMUPS, MAX_N = 1920, 1080, 30, 5, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", choices=("c2", "rtw"), required=True)
    args = ap.parse_args()
    import numpy as np
    import torch

    import __graft_entry__ as graft
    rt = graft.load_package()
    scene = rt.scene_prefix(rt.scene_builtin(1), 64) if args.frame == "c2" else rt.scene_builtin(2)
    cam = rt.camera_setup(scene, W, H)
    dev = rt.Device(0)
    dev.upload_scene(scene)
    stream = torch.cuda.current_stream().cuda_stream
    n = W * H
    mean = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    cur = torch.zeros(n, dtype=torch.int32, device="cuda")
    rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    hit = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    normal, albedo, out, scratch = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(4))
    rgba8 = torch.zeros(n, dtype=torch.int32, device="cuda")
    dev.trace(cam, width=W, height=H, prev_ptr=mean.data_ptr(), cur_ptr=cur.data_ptr(), rays_ptr=rays.data_ptr(),
              prev_count=0, frames=1, max_bounce=8, stream=stream)
    planes = dict(hit_ptr=hit.data_ptr(), normal_ptr=normal.data_ptr(), albedo_ptr=albedo.data_ptr())

    def first_hit():
        dev.trace_first_hit(cam, width=W, height=H, frame=0, stream=stream, **planes)

    def denoise(iterations, with_rgba8=False):
        rt.denoise(W, H, mean.data_ptr(), hit.data_ptr(), out.data_ptr(), scratch_ptr=scratch.data_ptr(),
                   normal_ptr=normal.data_ptr(), rgba8_ptr=rgba8.data_ptr() if with_rgba8 else 0, iterations=iterations,
                   stream=stream)

    def encode():
        rt.encode_rgba8(mean.data_ptr(), rgba8.data_ptr(), n, stream=stream)

    def timed(launch):
        for _ in range(WARMUPS):
            launch()
        torch.cuda.synchronize()
        us = []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        return dict(median=round(statistics.median(us), 1), min=round(min(us), 1), max=round(max(us), 1))

    first_hit()
    torch.cuda.synchronize()
    d = rt.denoise_defaults()
    res = dict(frame=args.frame, lib=os.environ.get("RT_TRACE_LIB", "librt_trace.so"), width=W, height=H, defaults=d,
               hit_pixels=int((hit[:, 0] != -1).sum().item()))
    res["first_hit_us"] = timed(first_hit)
    res["encode_us"] = timed(encode)
    res["total_us"] = {str(k): timed(lambda k=k: denoise(k)) for k in range(1, MAX_N + 1)}
    res["total_rgba8_us"] = timed(lambda: denoise(d["iterations"], True))
    res["encode_us_again"] = timed(encode)  # (the yardstick once more at the end: its drift over the run)
    # each pass against the streaming rate over its algorithmic bytes
    rate = n * 20 / res["encode_us"]["median"]  # bytes per microsecond
    pass_bytes = n * (16 + 16 + 8 + (16 if d["normal_power"] else 0))
    med = [0.0] + [res["total_us"][str(k)]["median"] for k in range(1, MAX_N + 1)]
    res["pass_us"] = [round(med[i + 1] - med[i], 1) for i in range(MAX_N)]
    res["stream_gb_per_s"] = round(rate / 1e3, 1)
    res["pass_bytes"] = pass_bytes
    res["pass_over_streaming"] = [round(p / (pass_bytes / rate), 2) for p in res["pass_us"]]
    denoise(d["iterations"], True)
    torch.cuda.synchronize()
    res["out_crc32"] = zlib.crc32(out.cpu().numpy().tobytes())
    res["rgba8_crc32"] = zlib.crc32(rgba8.cpu().numpy().tobytes())
    dev.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
