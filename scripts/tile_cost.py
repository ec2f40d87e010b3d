"""What rt_trace_tiles costs at C2 (1920x1080, 256 spp, 64 spheres, 8 bounces), by HIP events on
one GPU: (a) rt_trace, (b) rt_trace_tiles over all 2,040 tiles, (c) a 4x4-tile window over the
densest geometry (the window, on a 4-tile grid, whose pixels count the most segments).  Each is
timed warm, after its key's cold launch and two warm-ups (as bench.py does), median of the timed
steps.  Prints (b)/(a), and (c)'s time beside its share of the frame's segments and its lanes
per pixel.  Uses the library alone (no oracle, no reference).

usage: python scripts/tile_cost.py [--steps 5] [--spp 256]
"""
import argparse
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import __graft_entry__ as graft  # noqa: E402

W, H, N, B = 1920, 1080, 64, 8
WINDOW = 4  # tiles per window side


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=256)
    args = ap.parse_args()
    rt = graft.load_package()
    scene = rt.scene_prefix(rt.scene_builtin(1), N)
    cam = rt.camera_setup(scene, W, H)
    dev = rt.Device(0)
    dev.upload_scene(scene)
    dev.reserve(W, H)
    stream = torch.cuda.Stream()
    prev = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
    cur = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    ptrs = dict(width=W, height=H, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(), rays_ptr=rays.data_ptr(),
                max_bounce=B, accum_zero=True, stream=stream.cuda_stream)

    def launch(tiles, frames):
        if tiles is None:
            dev.trace(cam, frames=frames, **ptrs)
        else:
            dev.trace_tiles(cam, tiles=tiles, frames=frames, **ptrs)

    def segments(tiles, frames):
        rays.zero_()
        torch.cuda.synchronize()
        launch(tiles, frames)
        torch.cuda.synchronize()
        return int(rays.item())

    def timed(tiles):
        """(median ms, every ms, segments per launch, last_info) of warm launches of one key."""
        seg = segments(tiles, args.spp)  # the key's cold launch
        for _ in range(2):
            launch(tiles, args.spp)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for a, b in ev:
            a.record(stream)
            launch(tiles, args.spp)
            b.record(stream)
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in ev]
        return statistics.median(ms), ms, seg, dev.last_info()

    n_tiles = rt.tile_count(W, H)
    tiles_x = (W + rt.RT_TILE_SIZE - 1) // rt.RT_TILE_SIZE
    tiles_y = n_tiles // tiles_x
    # the densest window: segments of one frame per window of the 4-tile grid
    best = None
    for wy in range(0, tiles_y, WINDOW):
        for wx in range(0, tiles_x, WINDOW):
            t = rt.tiles_of_rect(W, H, wx * 32, wy * 32, (wx + WINDOW) * 32, (wy + WINDOW) * 32)
            s = segments(t, 1)
            if best is None or s > best[0]:
                best = (s, wx, wy, t)
    _, wx, wy, window = best

    out = {"workload": f"C2: {W}x{H}, {args.spp} spp, {N} spheres, {B} bounces", "steps": args.steps,
           "code_object_hash": rt.code_object_hash()}
    rows = []
    for name, tiles in (("rt_trace", None), ("rt_trace_tiles_all", list(range(n_tiles))), ("window_4x4", window)):
        ms, every, seg, info = timed(tiles)
        rows.append((name, ms, seg))
        out[name] = {"ms": round(ms, 4), "ms_steps": [round(v, 4) for v in every], "segments": seg,
                     "lanes_per_pixel": info["LanesPerPixel"], "tiles_selected": info["TilesSelected"],
                     "tiles_traced": info["TilesTraced"], "tiles_total": info["TilesTotal"]}
    a, b, c = rows
    assert a[2] == b[2], (a[2], b[2])  # a list of every tile counts rt_trace's segments
    out["all_tiles_over_rt_trace"] = round(b[1] / a[1], 4)
    out["window"] = {"tile_x": wx, "tile_y": wy, "tiles": len(window), "segment_share": round(c[2] / a[2], 5),
                     "time_share": round(c[1] / a[1], 5),
                     "pixel_share": round(len(window) * 1024 / (W * H), 5)}
    dev.close()
    print(json.dumps(out))
    print(f"rt_trace {a[1]:.3f} ms; all {n_tiles} tiles {b[1]:.3f} ms (x{b[1] / a[1]:.3f}); window {WINDOW}x{WINDOW} at "
          f"tile ({wx}, {wy}) {c[1]:.3f} ms = {100 * c[1] / a[1]:.1f} % of the frame's time for "
          f"{100 * c[2] / a[2]:.1f} % of its segments, {out['window_4x4']['lanes_per_pixel']} lanes per pixel")


if __name__ == "__main__":
    main()
