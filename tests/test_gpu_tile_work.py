"""GPU checks of rt_trace_tile_work: one launch over a list of the reference's 32 x 32 tiles in which
every tile carries its own (PreviousRayCount, Frames) pair.  Every pixel of a listed tile gets exactly
the bits of the full-frame `oracle.render` at that tile's pair, no other byte of either image is
written, the ray count and SegmentsFolded are the listed tiles' own, and the counts are no part of the
launch key.  Every comparison is bit-exact (no tolerance anywhere).

Base input (that of tests/test_gpu_tiles.py): scene 1 prefix 64, 136 x 104, 8 bounces: TilesX 5,
TilesY 4, the right column 8 px wide, the bottom row 8 px tall, tile 19 8 x 8.  Tiles 0, 5, 10, 14, 15
and 19 hold dead block tiles only (folded, not traced), tiles 1-3, 6-8, 11-13 mix live and dead ones.
Images start from a random running mean (continuations) with a poisoned RGBA8 image."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, B = 136, 104, 8
TILES_X, N_TILES = 5, 20
POISON = 0xDEADBEEF
POISON_I32 = POISON - (1 << 32)
OFF = -1
# block tile (2TW x 2TH) of a launch: by lanes per pixel, or 4 pixels per lane
BLOCK = {1: (16, 16), 2: (16, 8), 4: (8, 8), 8: (8, 4), 16: (4, 4), 32: (4, 2)}
MEAN = np.random.default_rng(2024).uniform(0.25, 2.0, (W * H, 4)).astype(np.float32)
MEAN.setflags(write=False)

# test 1's list: dead (0, 19: the 8 x 8 corner, 10), live and mixed tiles; Frames below every P > 1 (1, 2, 3)
# and beyond every ring size (40); fresh tiles (PreviousRayCount 0) beside continued ones
MIXED = {0: (0, 8), 7: (3, 4), 12: (3, 12), 19: (7, 1), 6: (7, 2), 13: (0, 40), 10: (5, 3)}


def tile_mask(w, h, tiles):
    """(h * w,) bool: the pixels of the listed tiles, each clipped to the image."""
    tx = (w + 31) // 32
    m = np.zeros((h, w), bool)
    for t in tiles:
        m[(t // tx) * 32:(t // tx) * 32 + 32, (t % tx) * 32:(t % tx) * 32 + 32] = True
    return m.ravel()


def block_tiles(w, h, tiles, info):
    """Block tiles of the launch's shape inside the listed tiles (rt_trace_info.TilesSelected)."""
    bw, bh = (32, 32) if info["PixelsPerLane"] == 4 else BLOCK[info["LanesPerPixel"]]
    tx, n = (w + 31) // 32, 0
    for t in tiles:
        cw, ch = min(32, w - (t % tx) * 32), min(32, h - (t // tx) * 32)
        n += -(-cw // bw) * -(-ch // bh)
    return n


def triples(work):
    return [(t, p, f) for t, (p, f) in work.items()]


class Images:
    """Both device images and the ray counter: the running mean given (default MEAN), RGBA8 poisoned."""

    def __init__(self, torch, w=W, h=H, mean=MEAN):
        self.torch, self.w, self.h, self.mean = torch, w, h, mean
        self.prev = torch.from_numpy(mean.copy()).to("cuda")
        self.cur = torch.full((w * h,), POISON_I32, dtype=torch.int32, device="cuda")
        self.rays = torch.zeros(1, dtype=torch.int64, device="cuda")

    def ptrs(self):
        return dict(prev_ptr=self.prev.data_ptr(), cur_ptr=self.cur.data_ptr(), rays_ptr=self.rays.data_ptr())

    def words(self):
        """(mean (h*w, 4) u32, RGBA8 (h*w,) u32, rays) after a device sync."""
        self.torch.cuda.synchronize()
        return (self.prev.view(self.torch.int32).cpu().numpy().view(np.uint32),
                self.cur.cpu().numpy().view(np.uint32), int(self.rays.item()))


def launch(dev, torch, cam, work, img, *, bounces=B, simd=True, srgb_pow=False):
    dev.trace_tile_work(cam, work=triples(work) if isinstance(work, dict) else work, width=img.w, height=img.h,
                        max_bounce=bounces, simd=simd, srgb_pow=srgb_pow,
                        stream=torch.cuda.current_stream().cuda_stream, **img.ptrs())


class Oracle:
    """Full-frame oracle renders of one scene / camera / size from one starting mean, cached per
    (PreviousRayCount, Frames) pair and read-only; `expected` takes each tile's pixels from the render
    of its own pair."""

    def __init__(self, orc, scene, cam, w, h, mean, bounces):
        self.orc, self.scene, self.cam, self.w, self.h, self.mean, self.bounces = orc, scene, cam, w, h, mean, bounces
        self.cache = {}

    def render(self, pair, simd=True):
        key = (pair, simd)
        if key not in self.cache:
            r = self.orc.render(self.scene, self.cam, self.w, self.h, prev_count=pair[0], frames=pair[1],
                                max_bounce=self.bounces, simd=simd, prev=self.mean.copy())
            r[0].setflags(write=False)
            r[1].setflags(write=False)
            self.cache[key] = r
        return self.cache[key]

    def expected(self, work, simd=True, srgb_pow=False):
        """(mean (h*w, 4) u32, RGBA8 (h*w,) u32, listed-pixel mask) of a launch over `work` from self.mean."""
        ep = self.mean.view(np.uint32).copy()
        ec = np.full(self.w * self.h, POISON, np.uint32)
        listed = np.zeros(self.w * self.h, bool)
        for t, pair in work.items():
            if pair[1] == 0:
                continue
            oprev, ocur, _ = self.render(tuple(pair), simd)
            m = tile_mask(self.w, self.h, [t])
            ep[m] = oprev.view(np.uint32)[m]
            ec[m] = self.orc.encode_rgba8(oprev[m], srgb_pow=True) if srgb_pow else ocur[m]
            listed |= m
        return ep, ec, listed


def assert_work(img, exp, what=""):
    """Listed tiles hold their pair's oracle words; every other word of both images is what it was."""
    ep, ec, listed = exp
    gp, gc, rays = img.words()
    assert listed.any()
    bad = np.flatnonzero((gp != ep).any(1))
    assert bad.size == 0, (f"{what}: {bad.size} pixels' means differ ({int(listed[bad].sum())} of them listed), "
                           f"first pixel {bad[0]} (tile {(bad[0] // img.w // 32) * ((img.w + 31) // 32) + bad[0] % img.w // 32})")
    badc = np.flatnonzero(gc != ec)
    assert badc.size == 0, f"{what}: {badc.size} RGBA8 pixels differ ({int(listed[badc].sum())} of them listed)"
    return rays


@pytest.fixture(scope="module")
def base(rt, orc, torch_cuda):
    """Scene, camera and the per-pair oracle renders of the base input (each computed once, read-only)."""
    s, o = rt.scene_prefix(rt.scene_builtin(1), 64), orc.scene_builtin(1).prefix(64)
    cam, ocam = rt.camera_setup(s, W, H), orc.camera(o, W, H)
    return dict(s=s, o=o, cam=cam, ocam=ocam, oracle=Oracle(orc, o, ocam, W, H, MEAN, B))


@pytest.fixture(scope="module")
def tdev(rt, torch_cuda, base):
    dev = rt.Device(0)
    dev.upload_scene(base["s"])
    yield dev
    dev.close()


# ------------------------------------------------- 1. mixed counts, parity and untouched bytes
def test_mixed_counts_match_and_nothing_else_is_written(torch_cuda, base, tdev):
    img = Images(torch_cuda)
    launch(tdev, torch_cuda, base["cam"], MIXED, img)
    assert_work(img, base["oracle"].expected(MIXED), "mixed")
    info = tdev.last_info()
    assert info["TileCounts"] == 1 and info["SplitHeadFrames"] == 0, info
    assert info["TilesSelected"] == block_tiles(W, H, list(MIXED), info) and info["TilesTotal"] > info["TilesSelected"]
    assert 0 < info["TilesTraced"] < info["TilesSelected"] and info["SegmentsFolded"] > 0, info
    assert info["LanesPerPixel"] == 16, info  # (a small window; never more lanes than the LARGEST Frames, 40)


# ------------------------------------------------- 2. ray counts against the oracle alone
ROW_PAIRS = [(0, 8), (3, 4), (3, 12), (7, 1)]


def dead_block_tiles(masks, info, w, h):
    """[(x0, y0, clipped w, clipped h)] of the launch's dead block tiles, from rt_debug_masks (16 groups:
    one word per wave tile): a block tile is dead when no wave tile inside the image has a candidate."""
    bw, bh = BLOCK[info["LanesPerPixel"]]
    tx, ty = -(-w // bw), -(-h // bh)
    assert masks.size == tx * ty * 4
    out = []
    for t in range(tx * ty):
        x0, y0 = (t % tx) * bw, (t // tx) * bh
        live = any(masks[4 * t + q] != 0 and x0 + (q & 1) * (bw // 2) < w and y0 + (q >> 1) * (bh // 2) < h
                   for q in range(4))
        if not live:
            out.append((x0, y0, min(bw, w - x0), min(bh, h - y0)))
    return out


def test_ray_counts_and_folded_segments(orc, torch_cuda, base, tdev):
    work = {t: ROW_PAIRS[t // TILES_X] for t in range(N_TILES)}
    img = Images(torch_cuda)
    launch(tdev, torch_cuda, base["cam"], work, img)
    rays = assert_work(img, base["oracle"].expected(work), "rows")
    want = sum(orc.render(base["o"], base["ocam"], W, H, prev_count=p, frames=f, max_bounce=B, prev=MEAN.copy(),
                          rows=(32 * r, min(H, 32 * r + 32)))[2] for r, (p, f) in enumerate(ROW_PAIRS))
    print("rays", rays, "oracle rows", want)
    assert rays == want
    info = tdev.last_info()
    assert info["TileCounts"] == 1 and info["TilesSelected"] == info["TilesTotal"], info
    dead = dead_block_tiles(tdev.debug_masks(max_words=1 << 16), info, W, H)
    folded = sum(cw * ch * ROW_PAIRS[y0 // 32][1] for _, y0, cw, ch in dead)
    print("SegmentsFolded", info["SegmentsFolded"], "from the masks", folded, "dead block tiles", len(dead))
    assert folded > 0 and info["SegmentsFolded"] == folded
    assert info["TilesTraced"] == info["TilesTotal"] - len(dead)


# ------------------------------------------------- 3. the counts are not in the key
SET_2 = {0: (8, 2), 7: (7, 16), 12: (15, 3), 19: (8, 5), 6: (9, 1), 13: (40, 20), 10: (8, 8)}
SET_3 = {0: (10, 6), 7: (23, 24), 12: (18, 7), 19: (13, 2), 6: (10, 3), 13: (60, 4), 10: (16, 1)}


def test_counts_are_not_in_the_key(rt, torch_cuda, base):
    assert list(SET_2) == list(SET_3) == list(MIXED)
    dev = rt.Device(0)
    try:
        dev.upload_scene(base["s"])
        infos = []
        for work in (MIXED, SET_2, SET_3):  # largest Frames 40, 20, 24: 16 lanes per pixel each time
            img = Images(torch_cuda)
            launch(dev, torch_cuda, base["cam"], work, img)
            assert_work(img, base["oracle"].expected(work), str(work))
            infos.append(dev.last_info())
        print([(i["CullPassRan"], i["OrderedLaunches"], i["PixelsSorted"]) for i in infos])
        assert [i["CullPassRan"] for i in infos] == [1, 0, 0]
        assert infos[0]["OrderedLaunches"] < infos[1]["OrderedLaunches"] < infos[2]["OrderedLaunches"]
        assert all(i["TileCounts"] == 1 and i["LanesPerPixel"] == 16 for i in infos)
        assert infos[0]["PixelsSorted"] == 0 and infos[2]["PixelsSorted"] == 1  # (16 lanes per pixel: the shape sorts)
        assert len({(i["TilesSelected"], i["TilesTraced"]) for i in infos}) == 1
        # the same tiles through rt_trace_tiles: the same key (16 frames: 16 lanes per pixel again)
        img = Images(torch_cuda)
        dev.trace_tiles(base["cam"], tiles=list(MIXED), width=W, height=H, prev_count=3, frames=16, max_bounce=B,
                        stream=torch_cuda.cuda.current_stream().cuda_stream, **img.ptrs())
        assert_work(img, base["oracle"].expected({t: (3, 16) for t in MIXED}), "rt_trace_tiles")
        info = dev.last_info()
        assert info["CullPassRan"] == 0 and info["TileCounts"] == 0 and info["PixelsSorted"] == 1, info
        # and back: still the key
        img = Images(torch_cuda)
        launch(dev, torch_cuda, base["cam"], MIXED, img)
        assert_work(img, base["oracle"].expected(MIXED), "again")
        assert dev.last_info()["CullPassRan"] == 0
    finally:
        dev.close()


# ------------------------------------------------- 4. uniform pairs are rt_trace_tiles
@pytest.mark.parametrize("pair,options,tiles", [((3, 8), {}, [0, 7, 12, 19]), ((5, 1), {}, [1, 7, 13, 19]),
                                                ((3, 64), {"HeadSamples": 1}, [7, 19])],
                         ids=["eight_frames", "one_frame", "split_first_launch"])
def test_uniform_pairs_are_rt_trace_tiles(rt, torch_cuda, base, pair, options, tiles):
    got = []
    for per_tile in (True, False):  # a fresh device each: both calls are their key's first launch
        dev = rt.Device(0, options=options)
        try:
            dev.upload_scene(base["s"])
            img = Images(torch_cuda)
            if per_tile:
                launch(dev, torch_cuda, base["cam"], {t: pair for t in tiles}, img)
            else:
                dev.trace_tiles(base["cam"], tiles=tiles, width=W, height=H, prev_count=pair[0], frames=pair[1],
                                max_bounce=B, stream=torch_cuda.cuda.current_stream().cuda_stream, **img.ptrs())
            rays = assert_work(img, base["oracle"].expected({t: pair for t in tiles}), f"per_tile={per_tile}")
            gp, gc, _ = img.words()
            got.append((gp, gc, rays, dev.last_info()))
        finally:
            dev.close()
    (ap, ac, ar, ai), (bp, bc, br, bi) = got
    assert np.array_equal(ap, bp) and np.array_equal(ac, bc) and ar == br
    assert {k: v for k, v in ai.items() if k != "TileCounts"} == {k: v for k, v in bi.items() if k != "TileCounts"}
    assert bi["TileCounts"] == 0 and ai["CullPassRan"] == 1
    if pair[1] == 1:
        assert ai["PixelsPerLane"] == 4 and ai["LanesPerPixel"] == 1, ai
    if options:
        assert ai["SplitHeadFrames"] > 0, ai


# ------------------------------------------------- 5. every launch shape and path
SHAPE_WORK = {1: (0, 8), 7: (3, 4), 13: (3, 12), 19: (7, 1)}  # live + dead block tiles, a live tile, the dead corner
ONE_FRAME_WORK = {1: (0, 1), 7: (3, 1), 13: (5, 1), 19: (7, 1)}
VARIANTS = [(f"lanes{p}", {"LanesPerPixel": p}, {}) for p in (1, 2, 4, 8, 16, 32)] + [
    ("one_frame_4_pixels_per_lane", {"PixelsPerLane": 4}, {"work": ONE_FRAME_WORK}),
    ("one_frame_default_device", {}, {"work": ONE_FRAME_WORK}),
    ("cull_off", {"Cull": OFF}, {}), ("four_wave_groups", {"OneWaveGroups": OFF}, {}),
    ("encode_pass_off", {"EncodePass": OFF}, {}), ("tile_order_off", {"TileOrder": OFF}, {}),
    ("pixel_sort_off", {"PixelSort": OFF}, {}), ("scalar_rules", {}, {"simd": False}),
    ("srgb_pow", {}, {"srgb_pow": True}),
    # four-wave devices whose kernels are not built with per-tile counts: the one-wave run-time kernel
    ("four_wave_sphere_source_lds", {"OneWaveGroups": OFF, "SphereSourceLds": 1}, {"routed": True}),
    ("four_wave_scene_in_hbm", {"OneWaveGroups": OFF, "SceneInHbm": 1}, {"routed": True}),
    ("walk_any", {"WalkAny": 1}, {})]


@pytest.mark.parametrize("name,options,how", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_every_launch_shape_and_path(rt, torch_cuda, base, name, options, how):
    work, simd, srgb_pow = how.get("work", SHAPE_WORK), how.get("simd", True), how.get("srgb_pow", False)
    exp = base["oracle"].expected(work, simd, srgb_pow)
    dev = rt.Device(0, options=options)
    try:
        dev.upload_scene(base["s"])
        for launch_no in range(3):  # a new key, the same key again (kept order), and once more (sorted pixels)
            img = Images(torch_cuda)
            launch(dev, torch_cuda, base["cam"], work, img, simd=simd, srgb_pow=srgb_pow)
            assert_work(img, exp, f"{name} launch {launch_no}")
            info = dev.last_info()
            assert info["TileCounts"] == 1 and info["SplitHeadFrames"] == 0, info
            assert info["CullPassRan"] == (1 if launch_no == 0 and name != "cull_off" else 0), info
            assert info["TilesSelected"] == block_tiles(W, H, list(work), info), info
            assert 0 < info["TilesTraced"] <= info["TilesSelected"], info
            if name == "cull_off":
                assert info["TilesTraced"] == info["TilesSelected"] and info["SegmentsFolded"] == 0, info
            else:
                assert info["SegmentsFolded"] > 0, info
            if "LanesPerPixel" in options:
                assert info["LanesPerPixel"] == options["LanesPerPixel"]
            if name.startswith("one_frame"):
                assert info["PixelsPerLane"] == 4
            if name == "four_wave_groups":
                assert info["OneWaveGroups"] == 0, info
            if how.get("routed"):
                assert info["OneWaveGroups"] == 1 and info["Walk"] == 0, info
    finally:
        dev.close()


# ------------------------------------------------- 6. the weight tables' edges
@pytest.mark.parametrize("options", [{}, {"OneWaveGroups": OFF}, {"OneWaveGroups": OFF, "LanesPerPixel": 4}],
                         ids=["default", "four_wave", "four_wave_fold_table_in_lds"])
def test_weight_table_edges(rt, torch_cuda, base, options):
    # 65530 + 12 crosses kWeightsN (65536: the one-wave kernels' static weight table), 250 + 12 crosses
    # kFoldTable (256: the four-wave kernels' LDS fold table at up to 8 lanes per pixel)
    work = {7: (65530, 12), 12: (250, 12), 1: (0, 12), 10: (65530, 12), 0: (250, 12)}
    dev = rt.Device(0, options=options)
    try:
        dev.upload_scene(base["s"])
        img = Images(torch_cuda)
        launch(dev, torch_cuda, base["cam"], work, img)
        assert_work(img, base["oracle"].expected(work), str(options))
        info = dev.last_info()
        assert info["TileCounts"] == 1 and info["OneWaveGroups"] == (0 if options else 1), info
    finally:
        dev.close()


# ------------------------------------------------- 7. other scenes
@pytest.mark.parametrize("scene,w,h,work", [
    (2, 72, 40, {0: (0, 2), 1: (2, 3), 2: (0, 2), 4: (2, 3), 5: (2, 3)}),  # RTWeekend: sky, nothing folds
    (0, 96, 72, {0: (0, 4), 2: (3, 2), 4: (0, 4), 6: (3, 2), 7: (3, 2), 8: (0, 4)}),  # RGB Glass: dead bottom tiles
], ids=["rtweekend", "rgb_glass"])
def test_other_scenes(rt, orc, torch_cuda, scene, w, h, work):
    s, o = rt.scene_builtin(scene), orc.scene_builtin(scene)
    cam, ocam = rt.camera_setup(s, w, h), orc.camera(o, w, h)
    mean = np.random.default_rng(7).uniform(0.25, 2.0, (w * h, 4)).astype(np.float32)
    oracle = Oracle(orc, o, ocam, w, h, mean, 5)
    dev = rt.Device(0)
    try:
        dev.upload_scene(s)
        img = Images(torch_cuda, w, h, mean)
        launch(dev, torch_cuda, cam, work, img, bounces=5)
        assert_work(img, oracle.expected(work), f"scene {scene}")
        info = dev.last_info()
        assert info["TileCounts"] == 1 and info["TilesSelected"] == block_tiles(w, h, list(work), info), info
        if o.use_sky:
            assert info["SegmentsFolded"] == 0 and info["TilesTraced"] == info["TilesSelected"], info
        else:
            assert info["SegmentsFolded"] > 0 and info["TilesTraced"] > 0, info
    finally:
        dev.close()


# ------------------------------------------------- 8. zero-frame entries
def test_zero_frame_entries_are_dropped(torch_cuda, base, tdev):
    work = {0: (0, 8), 5: (4, 0), 7: (3, 4), 8: (0, 0), 19: (7, 1), 10: (0xFFFFFFFF, 0)}
    kept = [t for t, (_, f) in work.items() if f]
    img = Images(torch_cuda)
    launch(tdev, torch_cuda, base["cam"], work, img)
    assert_work(img, base["oracle"].expected(work), "zero frames")  # (tiles 5, 8 and 10 keep every byte)
    info = tdev.last_info()
    assert info["TilesSelected"] == block_tiles(W, H, kept, info) and info["TileCounts"] == 1, info
    # nothing but zero-frame entries: nothing is enqueued
    img = Images(torch_cuda)
    launch(tdev, torch_cuda, base["cam"], {3: (0, 0), 4: (9, 0)}, img)
    gp, gc, rays = img.words()
    assert np.array_equal(gp, MEAN.view(np.uint32)) and np.all(gc == POISON) and rays == 0
    assert tdev.last_info()["TilesSelected"] == info["TilesSelected"]  # (the last launch is still that one)


# ------------------------------------------------- 9. errors
def _raw_call(rt, dev, cam, img, work, n_work=None, *, band_count=1):
    c = rt.RtCameraInfo()
    ctypes.pointer(c)[0] = cam
    c.CurrentImage = rt.RtImage(img.cur.data_ptr(), img.w, img.h, rt.RT_FORMAT_R8G8B8A8_U32)
    c.PreviousImage = rt.RtImage(img.prev.data_ptr(), img.w, img.h, rt.RT_FORMAT_R32B32G32A32_F32)
    # (PreviousRayCount / Frames of the desc are not read: values rt_trace itself would refuse)
    d = rt.RtTraceDesc(img.w, img.h, 0xFFFFFFFF, 0xFFFFFFFF, B, 1, rt.RT_SEED_PIXEL, 32, band_count, 0, 0)
    arr = None if work is None else rt.tile_work_array(work)
    n = n_work if n_work is not None else (0 if arr is None else arr.shape[0])
    return rt.lib().rt_trace_tile_work(dev.handle, ctypes.byref(c), ctypes.byref(d),
                                       ctypes.c_void_p(arr.ctypes.data if arr is not None and arr.size else None), n,
                                       ctypes.c_void_p(img.rays.data_ptr()),
                                       ctypes.c_void_p(img.torch.cuda.current_stream().cuda_stream))


def test_argument_errors_enqueue_nothing_and_leave_the_key(rt, torch_cuda, base):
    good = {7: (3, 4), 13: (0, 40), 19: (7, 1)}
    dev = rt.Device(0)
    try:
        dev.upload_scene(base["s"])
        img = Images(torch_cuda)
        launch(dev, torch_cuda, base["cam"], good, img)
        assert dev.last_info()["CullPassRan"] == 1
        bad_img = Images(torch_cuda)
        for what, work, kw in (("a tile listed twice", [(3, 0, 8), (9, 0, 8), (3, 1, 8)], {}),
                               ("a tile listed twice, once with no frames", [(3, 0, 8), (9, 0, 8), (3, 0, 0)], {}),
                               ("index 20", [(1, 0, 8), (20, 0, 8)], {}),
                               ("BandCount 2", triples(good), {"band_count": 2}),
                               ("NULL list", None, {"n_work": 2}),
                               ("a frame count past u32", [(7, 3, 4), (13, 0xFFFFFFFF, 1)], {})):
            rc = _raw_call(rt, dev, base["cam"], bad_img, work, **kw)
            assert rc == -22, (what, rc)
            assert rt.lib().rt_last_error(), what
            gp, gc, rays = bad_img.words()
            assert np.array_equal(gp, MEAN.view(np.uint32)) and np.all(gc == POISON) and rays == 0, what
            # the previous good call again: its key is still there
            img = Images(torch_cuda)
            launch(dev, torch_cuda, base["cam"], good, img)
            assert_work(img, base["oracle"].expected(good), what)
            assert dev.last_info()["CullPassRan"] == 0, what
        with pytest.raises(rt.RtError):
            launch(dev, torch_cuda, base["cam"], [(4, 0, 1), (4, 0, 2)], bad_img)
        assert _raw_call(rt, dev, base["cam"], bad_img, None, 0) == 0
        assert _raw_call(rt, dev, base["cam"], bad_img, triples(good), 0) == 0
        # the desc's own counts (here values rt_trace refuses) are not read
        img = Images(torch_cuda)
        assert _raw_call(rt, dev, base["cam"], img, triples(good)) == 0
        assert_work(img, base["oracle"].expected(good), "raw call")
        assert dev.last_info()["CullPassRan"] == 0
    finally:
        dev.close()


# ------------------------------------------------- 10. host array lifetime
def test_the_array_is_consumed_before_the_call_returns(rt, torch_cuda, base, tdev):
    work = {3: (3, 4), 8: (0, 8), 17: (7, 2)}
    arr = rt.tile_work_array(triples(work))
    img = Images(torch_cuda)
    c = rt.RtCameraInfo()
    ctypes.pointer(c)[0] = base["cam"]
    c.CurrentImage = rt.RtImage(img.cur.data_ptr(), W, H, rt.RT_FORMAT_R8G8B8A8_U32)
    c.PreviousImage = rt.RtImage(img.prev.data_ptr(), W, H, rt.RT_FORMAT_R32B32G32A32_F32)
    d = rt.RtTraceDesc(W, H, 0, 0, B, 1, rt.RT_SEED_PIXEL, 32, 1, 0, 0)
    rc = rt.lib().rt_trace_tile_work(tdev.handle, ctypes.byref(c), ctypes.byref(d), ctypes.c_void_p(arr.ctypes.data),
                                     arr.shape[0], ctypes.c_void_p(img.rays.data_ptr()),
                                     ctypes.c_void_p(torch_cuda.cuda.current_stream().cuda_stream))
    arr[:] = 0xFFFFFFFF  # before any sync
    assert rc == 0
    assert_work(img, base["oracle"].expected(work), "lifetime")


# ------------------------------------------------- 11. reservation
def test_reserve_covers_per_tile_launches(rt, torch_cuda, base):
    dev = rt.Device(0)
    try:
        dev.upload_scene(base["s"])
        dev.reserve(W, H)
        growths = dev.last_info()["BufferGrowths"]
        for work in (MIXED, SHAPE_WORK, {t: ROW_PAIRS[t // TILES_X] for t in range(N_TILES)}, ONE_FRAME_WORK, SET_2):
            img = Images(torch_cuda)
            launch(dev, torch_cuda, base["cam"], work, img)
            assert_work(img, base["oracle"].expected(work), str(work))
            info = dev.last_info()
            assert info["BufferGrowths"] == growths and info["TileCounts"] == 1, info
    finally:
        dev.close()


# ------------------------------------------------- 12. back to back
def test_back_to_back_calls_keep_their_own_counts(torch_cuda, base, tdev):
    works = (MIXED, SET_2, SET_3, MIXED)  # four tables through two staging slots, no sync in between
    imgs = [Images(torch_cuda) for _ in works]
    for img, work in zip(imgs, works):
        launch(tdev, torch_cuda, base["cam"], work, img)
    for img, work in zip(imgs, works):
        assert_work(img, base["oracle"].expected(work), str(work))
