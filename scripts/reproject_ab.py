"""HIP-event time of rt_reproject on one 1920 x 1080 frame beside the box's plain streaming pass (DESIGN.md §3,
"Carrying the mean across a camera move"): one frame per process.

  --frame c2 | rtw     scene 1 prefix 64 (the C2 frame) or scene 2 (RTWeekend)

The previous frame is the 1-spp running mean of rt_trace (8 bounces) at the scene's default camera with
rt_trace_first_hit's Hit plane at the pixel centre, carried once without history (Out = the mean, counts 1); the new
frame is the same pair one key step of 1/16 rad on.  Under the library's defaults the script times, each as 30 calls
after 5 warm-ups between two HIP events on one stream, median and range in microseconds:
  reproject         rt_reproject with history, no Rgba8
  reproject_rgba8   the same with Rgba8
  no_history        rt_reproject without history (a loop's first frame: Mean -> Out, the counts)
  encode            rt_encode_rgba8 over the same frame: 16 B read and 4 B written per pixel, the plain streaming pass;
                    its rate prices the pass's compulsory bytes -- Mean 16, Hit 8, History 16, HistoryHit 8,
                    HistoryCount 4 read once each and Out 16, OutCount 4 written: 72 B per pixel, 76 with Rgba8 -- and
                    over_streaming = time / (those bytes / that rate)
and prints one JSON line, with the share of hit pixels that carried their history and checksums of Out, OutCount
and Rgba8."""
import argparse
import json
import pathlib
import statistics
import sys
import zlib

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

W, H, CALLS, WARMUPS = 1920, 1080, 30, 5
BYTES, BYTES_RGBA8 = 72, 76


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
    history, out = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(2))
    history_count, out_count, rgba8 = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))

    def first_frame():
        rt.reproject(W, H, cams[0], cams[0], mean[0].data_ptr(), hit[0].data_ptr(), history.data_ptr(),
                     history_count.data_ptr(), stream=stream)

    def reproject(with_rgba8=False):
        rt.reproject(W, H, cams[1], cams[0], mean[1].data_ptr(), hit[1].data_ptr(), out.data_ptr(), out_count.data_ptr(),
                     history_ptr=history.data_ptr(), history_hit_ptr=hit[0].data_ptr(),
                     history_count_ptr=history_count.data_ptr(), rgba8_ptr=rgba8.data_ptr() if with_rgba8 else 0,
                     stream=stream)

    def encode():
        rt.encode_rgba8(mean[1].data_ptr(), rgba8.data_ptr(), n, stream=stream)

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

    first_frame()
    torch.cuda.synchronize()
    res = dict(frame=args.frame, width=W, height=H, defaults=rt.reproject_defaults(),
               hit_pixels=int((hit[1][:, 0] != -1).sum().item()))
    res["encode_us"] = timed(encode)
    res["reproject_us"] = timed(reproject)
    res["reproject_rgba8_us"] = timed(lambda: reproject(True))
    res["no_history_us"] = timed(first_frame)
    res["encode_us_again"] = timed(encode)  # (the yardstick once more at the end: its drift over the run)
    rate = n * 20 / res["encode_us"]["median"]  # bytes per microsecond
    res["stream_gb_per_s"] = round(rate / 1e3, 1)
    res["bytes_per_pixel"] = [BYTES, BYTES_RGBA8]
    res["streaming_us"] = [round(n * b / rate, 1) for b in (BYTES, BYTES_RGBA8)]
    res["over_streaming"] = [round(res["reproject_us"]["median"] / (n * BYTES / rate), 2),
                             round(res["reproject_rgba8_us"]["median"] / (n * BYTES_RGBA8 / rate), 2)]
    reproject(True)
    torch.cuda.synchronize()
    res["carried_pixels"] = int((out_count == 2).sum().item())
    res["out_crc32"] = zlib.crc32(out.cpu().numpy().tobytes())
    res["out_count_crc32"] = zlib.crc32(out_count.cpu().numpy().tobytes())
    res["rgba8_crc32"] = zlib.crc32(rgba8.cpu().numpy().tobytes())
    dev.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
