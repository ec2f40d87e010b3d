"""HIP-event time of rt_reproject_clip beside rt_reproject on one 1920 x 1080 frame ("Clamping the
carried history"): one frame per process.

  --frame c2 | rtw     scene 1 prefix 64 (the C2 frame) or scene 2 (RTWeekend)

The planes are scripts/reproject_ab.py's: the previous frame is the 1-spp running mean of rt_trace (8 bounces) at the
scene's default camera with rt_trace_first_hit's Hit plane at the pixel centre, carried once without history; the new
frame is the same pair one key step of 1/16 rad on.  Under the library's defaults (the default Gamma; the clamp's
cost does not depend on it) the script times, each as 30 calls after 5 warm-ups between two HIP events on one stream,
median and range in microseconds:
  reproject          rt_reproject with history, no Rgba8: the yardstick, in the same process
  encode             rt_encode_rgba8 over the same frame, the plain streaming pass
  clip_r1..3         rt_reproject_clip at Radius 1, 2, 3
  clip_no_history    rt_reproject_clip without history (a loop's first frame), beside rt_reproject's
  reproject_again    the yardstick once more at the end: its drift over the run
and prints one JSON line with each time's ratio to rt_reproject (the call reads no plane rt_reproject does not read,
so the ratio is the cost of the stencil), the share of carried pixels the clamp moved, and checksums of Out.
(profiles/reproject_clip_ab.txt also holds the run that had a second kernel shape, every tap a global load, under
the names direct_* and lds_*; lds is the kernel that stayed.)"""
import argparse
import json
import pathlib
import statistics
import sys
import zlib

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

W, H, CALLS, WARMUPS = 1920, 1080, 30, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", choices=("c2", "rtw"), required=True)
    args = ap.parse_args()
    import torch

    import __graft_entry__ as graft
    rt = graft.load_package()
    scene = rt.scene_prefix(rt.scene_builtin(1), 64) if args.frame == "c2" else rt.scene_builtin(2)
    cams = [rt.camera_setup(scene, W, H), rt.camera_setup(scene, W, H, x_angle=scene.DefaultXAngle + 1.0 / 16.0)]
    dev = rt.Device(0)
    dev.upload_scene(scene)
    stream = torch.cuda.current_stream().cuda_stream
    n = W * H
    cur = torch.zeros(n, dtype=torch.int32, device="cuda")
    rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    mean, hit = [], []
    for cam in cams:
        m = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        h = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        dev.trace(cam, width=W, height=H, prev_ptr=m.data_ptr(), cur_ptr=cur.data_ptr(), rays_ptr=rays.data_ptr(),
                  prev_count=0, frames=1, max_bounce=8, stream=stream)
        dev.trace_first_hit(cam, width=W, height=H, centre=True, hit_ptr=h.data_ptr(), stream=stream)
        mean.append(m)
        hit.append(h)
    history, out, plain = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(3))
    history_count, out_count, rgba8 = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
    rt.reproject(W, H, cams[0], cams[0], mean[0].data_ptr(), hit[0].data_ptr(), history.data_ptr(), history_count.data_ptr(),
                 stream=stream)
    planes = (W, H, cams[1], cams[0], mean[1].data_ptr(), hit[1].data_ptr())
    hist = dict(history_ptr=history.data_ptr(), history_hit_ptr=hit[0].data_ptr(), history_count_ptr=history_count.data_ptr())

    def reproject(**kw):
        rt.reproject(*planes, plain.data_ptr(), out_count.data_ptr(), stream=stream, **kw)

    def clip(radius, **kw):
        rt.reproject_clip(*planes, out.data_ptr(), out_count.data_ptr(), radius=radius, stream=stream, **kw)

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

    torch.cuda.synchronize()
    res = dict(frame=args.frame, width=W, height=H, defaults=rt.reproject_clip_defaults())
    res["encode_us"] = timed(lambda: rt.encode_rgba8(mean[1].data_ptr(), rgba8.data_ptr(), n, stream=stream))
    res["reproject_us"] = timed(lambda: reproject(**hist))
    for radius in (1, 2, 3):
        res[f"clip_r{radius}_us"] = timed(lambda: clip(radius, **hist))
    res["reproject_no_history_us"] = timed(reproject)
    res["clip_no_history_us"] = timed(lambda: clip(res["defaults"]["radius"]))
    res["reproject_again_us"] = timed(lambda: reproject(**hist))
    base = res["reproject_us"]["median"]
    res["ratio_to_reproject"] = {f"clip_r{radius}": round(res[f"clip_r{radius}_us"]["median"] / base, 2) for radius in (1, 2, 3)}
    res["out_crc32"] = {}
    for radius in (1, 2, 3):
        clip(radius, **hist)
        torch.cuda.synchronize()
        res["out_crc32"][f"clip_r{radius}"] = zlib.crc32(out.cpu().numpy().tobytes())
        carried = out_count.view(-1) == 2
        moved = ((out.view(torch.int32) != plain.view(torch.int32)).any(dim=1) & carried).sum().item()
        res[f"clamped_share_r{radius}"] = round(moved / max(int(carried.sum().item()), 1), 3)
    dev.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
