"""One side of the per-tile change statistics measurement: the workload of
scripts/tile_work_ab.py -- C2's scene and camera at 1920 x 1080, a work list over all 2040 reference
tiles in four equal groups by tile index mod 4 at (PreviousRayCount, Frames) = (0, 16), (16, 16),
(32, 32), (64, 64), every round, one call per round.

  --side plain  rt_trace_tile_work (also what an older library, RT_TRACE_LIB, can run)
  --side delta  rt_trace_tile_work_delta into a 2040-entry device array

Steady-state rounds are timed with HIP events around the whole round on one stream; prints one JSON
line: ms per round (median, min, max), segments per round (the ray counter's growth, the same every
round and on every side) and, for the delta side, the last round's statistics summed over the tiles.
scripts/gpu_tile_delta_ab.sh interleaves the sides.
"""
import argparse
import json
import os
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

GROUPS = [(0, 16), (16, 16), (32, 32), (64, 64)]
W, H, SPHERES, BOUNCES = 1920, 1080, 64, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=("plain", "delta"), required=True)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=6)
    args = ap.parse_args()
    import numpy as np
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
    delta = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    kw = dict(width=W, height=H, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(), rays_ptr=rays.data_ptr(),
              max_bounce=BOUNCES, stream=torch.cuda.current_stream().cuda_stream)
    if args.side == "delta":
        kw["delta_ptr"] = delta.data_ptr()
    work = [(t, *GROUPS[t % 4]) for t in range(n)]
    ms, segs, culls = [], [], 0
    for i in range(args.warmup + args.rounds):
        before = int(rays.item())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dev.trace_tile_work(cam, work=work, **kw)
        e1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            culls += dev.last_info()["CullPassRan"]
            ms.append(e0.elapsed_time(e1))
        segs.append(int(rays.item()) - before)
    assert len(set(segs)) == 1, segs  # a round's segments depend on the counts alone
    info = dev.last_info()
    med = statistics.median(ms)
    out = {"side": args.side, "lib": os.environ.get("RT_TRACE_LIB", "librt_trace.so"), "ms_per_round": round(med, 4),
           "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "segments_per_round": segs[0],
           "mrays_per_s": round(segs[0] / med / 1e3, 1), "rounds": args.rounds, "warmup": args.warmup,
           "cull_passes_in_timed_rounds": culls, "lanes_per_pixel": info["LanesPerPixel"],
           "tile_counts": info["TileCounts"]}
    if args.side == "delta":
        d = delta.cpu().numpy().view(np.uint32).reshape(n, 4).astype(np.uint64)
        out["delta_last_round"] = {"Changed": int(d[:, 0].sum()), "MaxDelta": int(d[:, 1].max()),
                                   "SumDelta": int(d[:, 2].sum()), "SumSquares": int(d[:, 3].sum())}
    print(json.dumps(out))
    dev.close()


if __name__ == "__main__":
    main()
