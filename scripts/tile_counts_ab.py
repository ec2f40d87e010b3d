"""One side of the device-table measurement: an adaptive refinement run on C2's scene and camera at
1920 x 1080 with all 2040 reference tiles listed, in four equal groups (510 tiles each, by tile index mod 4) that
start at (PreviousRayCount, Frames) = (1, 1), (2, 2), (4, 4), (8, 8); eight rounds, each doubling the sample count of
the tiles still moving; a tile rests once a round moved none of its R, G, B bytes by more than 1.

  --side host    Level 2c: per round one rt_trace_tile_work_delta call, a 32 KB copy of the statistics, a stream
                 synchronisation, the rule on the CPU (numpy, vectorised) and a new work list
  --side device  Level 2d: per round rt_trace_tile_counts + rt_tile_counts_step + one asynchronous 16-byte summary
                 copy; the host waits once, after the last round

A run is timed start to finish on one stream by the host's clock (the host's waits and work are what is measured),
after a warm-up run; a counting run reads rt_trace_info after every round (cull passes, which waits) and is not
timed.  Prints one JSON line: ms per round (median, min, max over the timed runs' total / rounds), host
synchronisations per round, cull passes over a run, tiles at rest after each round, and the final table's checksum
(the same on both sides).  scripts/gpu_tile_counts_ab.sh interleaves the two sides.
"""
import argparse
import json
import pathlib
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

START = [(1, 1), (2, 2), (4, 4), (8, 8)]
W, H, SPHERES, BOUNCES = 1920, 1080, 64, 8
ROUNDS, MAX_ROUND, MAX_TILE, REST_MAX_DELTA, U32 = 8, 1024, 0xFFFFFFFF, 1, 0xFFFFFFFF


def rule_numpy(counts, delta):
    """rt_tile_counts_step on the host (rt_trace.h): the new (n, 2) table and the tiles still active."""
    prev, frames = counts[:, 0].astype(np.int64), counts[:, 1].astype(np.int64)
    f = np.minimum(frames, MAX_ROUND)
    f = np.where(prev + f > U32, 0, f)
    ran = f > 0
    done = prev + f
    rest = (done >= MAX_TILE) | ((prev != 0) & (delta[:, 1] <= REST_MAX_DELTA))
    nxt = np.where(rest, 0, np.minimum(np.minimum(done, MAX_ROUND), MAX_TILE - done))
    out = counts.copy()
    out[ran, 0] = done[ran]
    out[ran, 1] = nxt[ran]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=("host", "device"), required=True)
    ap.add_argument("--runs", type=int, default=5)
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
    delta = torch.zeros(n * 4, dtype=torch.int32, device="cuda")
    h_delta = torch.zeros(n * 4, dtype=torch.int32).pin_memory()
    start = np.array([START[t % 4] for t in range(n)], np.uint32)
    d_start = torch.from_numpy(start.view(np.int32).copy()).to("cuda")
    table = torch.zeros_like(d_start)
    d_summary = torch.zeros(4, dtype=torch.int32, device="cuda")
    h_summary = torch.zeros((ROUNDS, 4), dtype=torch.int32).pin_memory()
    stream = torch.cuda.current_stream().cuda_stream
    kw = dict(width=W, height=H, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(), rays_ptr=rays.data_ptr(),
              max_bounce=BOUNCES, stream=stream)
    tiles = np.arange(n, dtype=np.uint32)
    rule = rt.tile_rule(MAX_ROUND, MAX_TILE, REST_MAX_DELTA, U32)

    def run(count_culls):
        """One refinement run from the start state: (seconds, cull passes, resting tiles per round, final table)."""
        prev.zero_()
        cur.zero_()
        rays.zero_()
        table.copy_(d_start)
        torch.cuda.synchronize()
        culls, resting, syncs = 0, [], 0
        t0 = time.perf_counter()
        if args.side == "host":
            counts = start.copy()
            for _ in range(ROUNDS):
                live = np.flatnonzero(counts[:, 1])
                if live.size:
                    work = np.concatenate([live[:, None].astype(np.uint32), counts[live]], 1)
                    dev.trace_tile_work(cam, work=work, delta_ptr=delta.data_ptr(), **kw)
                    culls += dev.last_info()["CullPassRan"] if count_culls else 0
                h_delta.copy_(delta, non_blocking=True)
                torch.cuda.current_stream().synchronize()
                syncs += 1
                counts = rule_numpy(counts, h_delta.numpy().view(np.uint32).reshape(-1, 4))
                resting.append(int((counts[:, 1] == 0).sum()))
            final = counts
        else:
            for r in range(ROUNDS):
                dev.trace_tile_counts(cam, tiles=tiles, counts_ptr=table.data_ptr(), max_frames=MAX_ROUND,
                                      delta_ptr=delta.data_ptr(), **kw)
                culls += dev.last_info()["CullPassRan"] if count_culls else 0
                rt.tile_counts_step(table.data_ptr(), delta.data_ptr(), W, H, rule, d_summary.data_ptr(), stream)
                h_summary[r].copy_(d_summary, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            syncs += 1
            s = h_summary.numpy().view(rt.tile_step_summary_dtype).reshape(-1)
            resting = [n - int(x["ActiveTiles"]) for x in s]
            final = table.cpu().numpy().view(np.uint32)
        sec = time.perf_counter() - t0
        return sec, culls, resting, final, syncs, int(rays.item())

    run(False)  # warm-up: the clocks, the first key's cull pass and order
    _, culls, resting, final, syncs, segs = run(True)
    ms = [run(False)[0] * 1e3 / ROUNDS for _ in range(args.runs)]
    print(json.dumps({"side": args.side, "ms_per_round": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                      "ms_max": round(max(ms), 4), "rounds": ROUNDS, "runs": args.runs,
                      "host_syncs_per_round": round(syncs / ROUNDS, 3), "cull_passes_per_run": culls,
                      "tiles_resting_after_round": resting, "segments_per_run": segs,
                      "final_table_crc32": zlib.crc32(np.ascontiguousarray(final).tobytes())}))
    dev.close()


if __name__ == "__main__":
    main()
