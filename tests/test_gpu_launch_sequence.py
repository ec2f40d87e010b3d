"""What one launch leaves behind for the next: a sequence of launches on ONE device, in which every
call meets the state of the calls before it -- the tile key and its two pinned upload slots, the learned
order, the asynchronous totals, the grown buffers, the last-launch record.

Device options {"HeadSamples": 1, "LanesPerPixel": 4}: a 64 x 48 image has 3072 pixels, far below 3072
per CU of a 256-CU device, so the lanes-per-pixel rule alone picks 16 lanes and a 16-frame launch never
reaches the split's minimum (4 x HeadSamples x lanes); at 4 lanes it is exactly that minimum and splits.
64 x 48: 2 x 2 reference tiles, the bottom row 16 pixels high.  Scene 1's 64-sphere prefix, 8 bounces.

After every step the running mean and the RGBA8 image equal the oracle's, bit for bit, for the frames
traced so far (every listed tile's pixels from the full-frame oracle render of the tile's own pair, every
other pixel untouched), and rt_trace_last_info's fields equal literals.  The ray counter equals the
oracle's sum wherever the oracle has it -- the launches that cover whole rows of the image; the oracle
counts rays by rows, not by tiles -- and a literal after a tile step.  Every literal is what the parent
commit's library printed for this same sequence on an MI355X (profiles/r17a_launch_sequence_parent.txt;
`python tests/test_gpu_launch_sequence.py` prints the record of the library RT_TRACE_LIB names)."""
import numpy as np
import pytest

W, H, B = 64, 48, 8
W2, H2 = 96, 64
OPTIONS = {"HeadSamples": 1, "LanesPerPixel": 4}
FIELDS = ("LanesPerPixel", "PixelsPerLane", "TilesTotal", "TilesSelected", "CullPassRan", "OrderedLaunches",
          "SplitHeadFrames", "OneWaveGroups", "Walk", "ClusteredWalk")

# (name, kind, image, arguments).  trace: (PreviousRayCount, Frames); tiles: (list, PreviousRayCount, Frames);
# work / delta: {tile: (PreviousRayCount, Frames)}; scene: spheres of scene 1's prefix to upload first
STEPS = [
    ("trace16", "trace", 0, (0, 16)),                                   # new key, split first launch
    ("trace16_again", "trace", 0, (16, 16)),                            # same key, a re-sort
    ("tiles_0_3", "tiles", 0, ([0, 3], 32, 4)),
    ("tiles_1", "tiles", 0, ([1], 32, 4)),                              # a new key through the other pinned slot
    ("tiles_0_3_again", "tiles", 0, ([0, 3], 36, 4)),
    ("work_mixed", "work", 0, {0: (40, 2), 1: (36, 6), 3: (40, 2)}),
    ("work_other_counts", "work", 0, {0: (42, 1), 1: (42, 2), 3: (42, 3)}),  # same key, new table
    ("work_delta_uniform", "delta", 0, {0: (45, 2), 1: (45, 2), 3: (45, 2)}),
    ("scene16_trace", "scene", 0, 16),
    ("scene16_trace", "trace", 0, (47, 16)),                            # a new scene generation
    ("larger_image", "trace", 1, (0, 16)),                              # buffer growth, the key cleared
    ("first_again", "trace", 0, (63, 16)),
]

# name: (the FIELDS of rt_trace_last_info, TileCounts, the ray counter of the step's image afterwards)
PARENT = {
    "trace16": ((4, 1, 48, 48, 1, 0, 4, 1, 2, 1), 0, 66085),
    "trace16_again": ((4, 1, 48, 48, 0, 2, 0, 1, 2, 1), 0, 132282),
    "tiles_0_3": ((4, 1, 48, 24, 1, 0, 0, 1, 2, 1), 0, 139569),
    "tiles_1": ((4, 1, 48, 16, 1, 0, 0, 1, 2, 1), 0, 146404),
    "tiles_0_3_again": ((4, 1, 48, 24, 1, 0, 0, 1, 2, 1), 0, 153720),  # (only the last key is kept)
    "work_mixed": ((4, 1, 48, 40, 1, 0, 0, 1, 2, 1), 1, 167668),
    "work_other_counts": ((4, 1, 48, 40, 0, 1, 0, 1, 2, 1), 1, 174137),
    "work_delta_uniform": ((4, 1, 48, 40, 0, 2, 0, 1, 2, 1), 0, 181183),
    "scene16_trace": ((4, 1, 48, 48, 1, 0, 4, 1, 2, 1), 0, 244248),
    "larger_image": ((4, 1, 96, 96, 1, 0, 4, 1, 2, 1), 0, 126710),
    "first_again": ((4, 1, 48, 48, 1, 0, 4, 1, 2, 1), 0, 307337),
}


def tile_mask(w, h, tiles):
    tx = (w + 31) // 32
    m = np.zeros((h, w), bool)
    for t in tiles:
        m[(t // tx) * 32:(t // tx) * 32 + 32, (t % tx) * 32:(t % tx) * 32 + 32] = True
    return m.ravel()


def run_sequence(rt, torch, after_step):
    """Runs STEPS on one device; after_step(name, kind, image index, arguments, n_spheres, info, images) follows
    every launch, with images = (prev, cur, rays) device tensors of the step's image."""
    stream = torch.cuda.current_stream().cuda_stream
    scene1 = rt.scene_builtin(1)
    n_spheres = 64
    scene = rt.scene_prefix(scene1, n_spheres)
    cams = [rt.camera_setup(scene, W, H), rt.camera_setup(scene, W2, H2)]
    sizes = [(W, H), (W2, H2)]
    images = [(torch.zeros((w * h, 4), dtype=torch.float32, device="cuda"),
               torch.zeros(w * h, dtype=torch.int32, device="cuda"),
               torch.zeros(1, dtype=torch.int64, device="cuda")) for w, h in sizes]
    delta = torch.zeros(rt.tile_count(W, H) * 4, dtype=torch.int32, device="cuda")
    dev = rt.Device(0, options=OPTIONS)
    try:
        dev.upload_scene(scene)
        for name, kind, im, args in STEPS:
            if kind == "scene":
                n_spheres = args
                scene = rt.scene_prefix(scene1, n_spheres)
                dev.upload_scene(scene)
                continue
            (w, h), (prev, cur, rays) = sizes[im], images[im]
            common = dict(width=w, height=h, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(), rays_ptr=rays.data_ptr(),
                          max_bounce=B, stream=stream)
            if kind == "trace":
                dev.trace(cams[im], prev_count=args[0], frames=args[1], **common)
            elif kind == "tiles":
                dev.trace_tiles(cams[im], tiles=args[0], prev_count=args[1], frames=args[2], **common)
            else:
                dev.trace_tile_work(cams[im], work=[(t, p, f) for t, (p, f) in args.items()],
                                    delta_ptr=delta.data_ptr() if kind == "delta" else 0, **common)
            torch.cuda.synchronize()
            after_step(name, kind, im, args, n_spheres, dev.last_info(), images[im])
    finally:
        dev.close()


def record(info, rays):
    return tuple(info[f] for f in FIELDS), info["TileCounts"], int(rays.item())


@pytest.mark.gpu
def test_launch_sequence_on_one_device(rt, orc, torch_cuda):
    from test_gpu_parity import assert_same
    sizes = [(W, H), (W2, H2)]
    oscene1 = orc.scene_builtin(1)
    # the oracle's state: per image the running mean, the RGBA8 image and the rays of the launches so far
    state = [[np.zeros((w * h, 4), np.float32), np.zeros(w * h, np.uint32), 0] for w, h in sizes]

    def after_step(name, kind, im, args, n_spheres, info, images):
        w, h = sizes[im]
        osc = oscene1.prefix(n_spheres)
        ocam = orc.camera(oscene1.prefix(64), w, h)  # (the camera of the sequence: the first scene's)
        mean, cur, rays = state[im]
        got = record(info, images[2])
        print(name, got)
        if kind == "trace":
            mean, cur, r = orc.render(osc, ocam, w, h, prev_count=args[0], frames=args[1], max_bounce=B, prev=mean.copy())
            rays += r
        else:
            work = {t: (args[1], args[2]) for t in args[0]} if kind == "tiles" else args
            new_mean, new_cur = mean.copy(), cur.copy()
            for t, (p, f) in work.items():
                omean, ocur, _ = orc.render(osc, ocam, w, h, prev_count=p, frames=f, max_bounce=B, prev=mean.copy())
                m = tile_mask(w, h, [t])
                new_mean[m], new_cur[m] = omean[m], ocur[m]
            mean, cur = new_mean, new_cur
            rays = PARENT[name][2]  # (the oracle counts rays by rows, not by tiles: the parent's count)
        state[im] = [mean, cur, rays]
        assert_same(images[0], images[1], got[2], mean, cur, rays)
        assert got == PARENT[name], (name, got, PARENT[name])

    run_sequence(rt, torch_cuda, after_step)


if __name__ == "__main__":  # the record of this sequence under the library RT_TRACE_LIB names
    import pathlib
    import sys

    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
    import torch

    import __graft_entry__ as graft

    pkg = graft.load_package()
    print("library", pkg.LIB_PATH.name, "code_object_hash", pkg.code_object_hash())
    print("fields", *FIELDS, "TileCounts", "rays", "mean_hash", "rgba8_hash")

    def show(name, kind, im, args, n_spheres, info, images):
        print(f'    "{name}": {record(info, images[2])},', f"# {pkg.frame_hash(images[0].cpu().numpy()):016x}",
              f"{pkg.frame_hash(images[1].cpu().numpy()):016x}", flush=True)

    run_sequence(pkg, torch, show)
