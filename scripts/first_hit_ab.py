"""HIP-event time of rt_trace_first_hit beside the trace launch that does the same primary work (DESIGN.md §3,
"The first hit as a pass of its own"): one frame at 1920 x 1080, one variant per process.

  --frame c2 | rtw     scene 1 prefix 64 (the C2 frame) or scene 2 (RTWeekend), the scene's default camera
  --variant all        Hit, Normal and Albedo
            hit        Hit alone
            cull_off   all three planes on a device created with Cull off (every pair of every group tested)
            trace      the yardstick: rt_trace with Frames = 1, MaxBounce = 1, RT_FLAG_ACCUM_ZERO on the same frame,
                       timed once its key has settled (after OrderLaunches + 2 launches): the same primary rays and
                       pair tests, plus the fold and the RGBA8 store

20 launches after 3 warm-ups (the yardstick: after its key has settled), each between two HIP events on one stream;
prints one JSON line with the median and the range in microseconds and, for the first-hit variants, the hit pixels
and a checksum of the Key plane (the same for all, hit and cull_off).  scripts/gpu_first_hit_ab.sh runs the matrix."""
import argparse
import json
import pathlib
import statistics
import sys
import zlib

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

W, H, LAUNCHES, WARMUPS = 1920, 1080, 20, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", choices=("c2", "rtw"), required=True)
    ap.add_argument("--variant", choices=("all", "hit", "cull_off", "trace"), required=True)
    args = ap.parse_args()
    import numpy as np
    import torch

    import __graft_entry__ as graft
    rt = graft.load_package()
    scene = rt.scene_prefix(rt.scene_builtin(1), 64) if args.frame == "c2" else rt.scene_builtin(2)
    cam = rt.camera_setup(scene, W, H)
    dev = rt.Device(0, options={"Cull": rt.RT_OPT_OFF} if args.variant == "cull_off" else None)
    dev.upload_scene(scene)
    stream = torch.cuda.current_stream().cuda_stream
    out = dict(frame=args.frame, variant=args.variant, width=W, height=H)
    if args.variant == "trace":
        prev = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
        cur = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        rays = torch.zeros(1, dtype=torch.int64, device="cuda")

        def launch():
            dev.trace(cam, width=W, height=H, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(), rays_ptr=rays.data_ptr(),
                      prev_count=0, frames=1, max_bounce=1, accum_zero=True, stream=stream)
        warmups = WARMUPS + 6  # (OrderLaunches is 4 by default: the key's order is kept by then)
    else:
        hit = torch.zeros((W * H, 2), dtype=torch.int32, device="cuda")
        normal = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
        albedo = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
        planes = dict(hit_ptr=hit.data_ptr())
        if args.variant != "hit":
            planes.update(normal_ptr=normal.data_ptr(), albedo_ptr=albedo.data_ptr())

        def launch():
            dev.trace_first_hit(cam, width=W, height=H, frame=0, stream=stream, **planes)
        warmups = WARMUPS
    for _ in range(warmups):
        launch()
    torch.cuda.synchronize()
    us = []
    for _ in range(LAUNCHES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    out.update(us_median=round(statistics.median(us), 1), us_min=round(min(us), 1), us_max=round(max(us), 1))
    if args.variant == "trace":
        info = dev.last_info()
        out.update(lanes_per_pixel=info["LanesPerPixel"], pixels_per_lane=info["PixelsPerLane"],
                   ordered_launches=info["OrderedLaunches"], rays=int(rays.item()) // (warmups + LAUNCHES))
    else:
        key = hit.cpu().numpy().view(np.uint32)[:, 0]
        out.update(hit_pixels=int((key != rt.HIT_MISS).sum()), key_crc32=zlib.crc32(key.tobytes()))
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
