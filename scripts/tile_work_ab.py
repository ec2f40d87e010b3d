"""One side of the per-tile work measurement: C2's scene and camera at 1920 x 1080, a
work list over all 2040 reference tiles in four equal groups by tile index mod 4 at (PreviousRayCount,
Frames) = (0, 16), (16, 16), (32, 32), (64, 64), every round.

  --side work   one rt_trace_tile_work call per round
  --side tiles  four rt_trace_tiles calls per round (one per group: what a caller did before)

Steady-state rounds are timed with HIP events around the whole round on one stream; prints one JSON
line: ms per round (median, min, max), segments per round (the ray counter's growth, the same every
round and on both sides) and Mrays/s.  scripts/gpu_tile_work_ab.sh interleaves the two sides.
"""
import argparse
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

GROUPS = [(0, 16), (16, 16), (32, 32), (64, 64)]
W, H, SPHERES, BOUNCES = 1920, 1080, 64, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=("work", "tiles"), required=True)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=6)
    args = ap.parse_args()
    import torch

    import __graft_entry__ as graft
    rt = graft.load_package()
    scene = rt.scene_prefix(rt.scene_builtin(1), SPHERES)
    cam = rt.camera_setup(scene, W, H)
    n = rt.tile_count(W, H)
    assert n == 2040
    dev = rt.Device(0)
    dev.upload_scene(scene)
    dev.reserve(W, H)
    prev = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    cur = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    kw = dict(width=W, height=H, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(), rays_ptr=rays.data_ptr(),
              max_bounce=BOUNCES, stream=stream)
    work = [(t, *GROUPS[t % 4]) for t in range(n)]
    lists = [[t for t in range(n) if t % 4 == g] for g in range(4)]

    def one_round():
        if args.side == "work":
            dev.trace_tile_work(cam, work=work, **kw)
        else:
            for g, (p, f) in enumerate(GROUPS):
                dev.trace_tiles(cam, tiles=lists[g], prev_count=p, frames=f, **kw)

    ms, segs, culls = [], [], 0
    for i in range(args.warmup + args.rounds):
        before = int(rays.item())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        one_round()
        e1.record()
        torch.cuda.synchronize()
        culls += dev.last_info()["CullPassRan"] if i >= args.warmup else 0
        if i >= args.warmup:
            ms.append(e0.elapsed_time(e1))
        segs.append(int(rays.item()) - before)
    assert len(set(segs)) == 1, segs  # a round's segments depend on the counts alone
    info = dev.last_info()
    med = statistics.median(ms)
    print(json.dumps({"side": args.side, "ms_per_round": round(med, 4), "ms_min": round(min(ms), 4),
                      "ms_max": round(max(ms), 4), "segments_per_round": segs[0],
                      "mrays_per_s": round(segs[0] / med / 1e3, 1), "rounds": args.rounds, "warmup": args.warmup,
                      "last_call_cull_passes_in_timed_rounds": culls, "lanes_per_pixel": info["LanesPerPixel"],
                      "tile_counts": info["TileCounts"]}))
    dev.close()


if __name__ == "__main__":
    main()
