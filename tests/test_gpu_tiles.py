"""GPU checks of rt_trace_tiles: a launch over a list of the reference's 32 x 32
tiles gives every pixel of a listed tile exactly the bits of the full-frame
render and writes no other byte of either image; its ray count is the listed
tiles' alone.  Every comparison is bit-exact against `oracle.render` of the
FULL frame (no tolerance anywhere); images start from a poison pattern so that
an untouched word is recognisable.

Base input: scene 1 prefix 64, 136 x 104, 8 frames, 8 bounces: TilesX 5,
TilesY 4, the right column 8 px wide, the bottom row 8 px tall, tile 19 8 x 8.
The frame counts 151,894 segments, tile row 0 51,026.  Tiles 0, 5, 10, 14, 15
and 19 hold dead block tiles only (no sphere's cone test passes: folded, not
traced), tiles 1-3, 6-8, 11-13 mix live and dead block tiles."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, F, B = 136, 104, 8, 8
TILES_X, N_TILES = 5, 20
FULL_RAYS, ROW0_RAYS = 151894, 51026
ALL = list(range(N_TILES))
POISON = 0xDEADBEEF
POISON_I32 = POISON - (1 << 32)
OFF = -1
# block tile (2TW x 2TH) of a launch: by lanes per pixel, or 4 pixels per lane
BLOCK = {1: (16, 16), 2: (16, 8), 4: (8, 8), 8: (8, 4), 16: (4, 4), 32: (4, 2)}

LISTS = {"7": [7], "0": [0], "19": [19], "right_column": [4, 9, 14, 19], "bottom_row": [15, 16, 17, 18, 19],
         "even": ALL[0::2], "all_but_7": [t for t in ALL if t != 7], "descending": [18, 13, 12, 7, 3, 1]}


def complement(tiles, n=N_TILES):
    return [t for t in range(n) if t not in tiles]


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


class Images:
    """Both device images and the ray counter; poisoned, or started from a given running mean."""

    def __init__(self, torch, w, h, mean=None):
        self.torch, self.w, self.h = torch, w, h
        if mean is None:
            self.prev = torch.full((w * h, 4), POISON_I32, dtype=torch.int32, device="cuda").view(torch.float32)
        else:
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


def launch(dev, torch, cam, tiles, img, *, frames=F, bounces=B, prev_count=0, simd=True, srgb_pow=False):
    dev.trace_tiles(cam, tiles=tiles, width=img.w, height=img.h, prev_count=prev_count, frames=frames,
                    max_bounce=bounces, simd=simd, srgb_pow=srgb_pow, stream=torch.cuda.current_stream().cuda_stream,
                    **img.ptrs())


def assert_tiles(img, tiles, oprev, ocur, *, mean_before=None):
    """Listed tiles hold the oracle's words; every other word of both images is what it was."""
    gp, gc, rays = img.words()
    m = tile_mask(img.w, img.h, tiles)
    op = oprev.reshape(-1, 4).view(np.uint32)
    oc = ocur.reshape(-1)
    assert m.any()
    bad = np.flatnonzero((gp[m] != op[m]).any(1))
    assert bad.size == 0, f"{bad.size} listed pixels' means differ, first pixel {np.flatnonzero(m)[bad[0]]}"
    assert np.array_equal(gc[m], oc[m]), f"{int((gc[m] != oc[m]).sum())} listed RGBA8 pixels differ"
    before = POISON if mean_before is None else mean_before.view(np.uint32)[~m]
    assert np.all(gp[~m] == before), f"{int((gp[~m] != before).any(1).sum())} unlisted pixels' means were written"
    assert np.all(gc[~m] == POISON), f"{int((gc[~m] != POISON).sum())} unlisted RGBA8 pixels were written"
    return rays


@pytest.fixture(scope="module")
def base(rt, orc, torch_cuda):
    """Scene, camera and the full-frame oracle renders of the base input (computed once, read-only)."""
    s, o = rt.scene_prefix(rt.scene_builtin(1), 64), orc.scene_builtin(1).prefix(64)
    cam, ocam = rt.camera_setup(s, W, H), orc.camera(o, W, H)
    cache = {}

    def oracle(frames=F, simd=True):
        if (frames, simd) not in cache:
            r = orc.render(o, ocam, W, H, frames=frames, max_bounce=B, simd=simd)
            r[0].setflags(write=False)
            r[1].setflags(write=False)
            cache[(frames, simd)] = r
        return cache[(frames, simd)]

    assert oracle()[2] == FULL_RAYS
    assert orc.render(o, ocam, W, H, frames=F, max_bounce=B, rows=(0, 32))[2] == ROW0_RAYS
    return dict(s=s, o=o, cam=cam, ocam=ocam, oracle=oracle)


@pytest.fixture(scope="module")
def tdev(rt, torch_cuda, base):
    dev = rt.Device(0)
    dev.upload_scene(base["s"])
    yield dev
    dev.close()


# ------------------------------------------------- 1. parity and untouched bytes
@pytest.mark.parametrize("name", list(LISTS))
def test_listed_tiles_match_and_nothing_else_is_written(torch_cuda, base, tdev, name):
    tiles = LISTS[name]
    img = Images(torch_cuda, W, H)
    launch(tdev, torch_cuda, base["cam"], tiles, img)
    oprev, ocur, _ = base["oracle"]()
    assert_tiles(img, tiles, oprev, ocur)
    info = tdev.last_info()
    assert info["TilesSelected"] == block_tiles(W, H, tiles, info) and info["TilesTotal"] > info["TilesSelected"]
    if name in ("0", "19", "bottom_row"):  # dead tiles only, or some: the fold ran, over selected tiles alone
        assert info["SegmentsFolded"] > 0, info
        assert info["SegmentsFolded"] <= int(tile_mask(W, H, tiles).sum()) * F
    if name in ("0", "19"):
        assert info["TilesTraced"] == 0 and info["SegmentsFolded"] == int(tile_mask(W, H, tiles).sum()) * F, info
    if name in ("7", "even", "all_but_7", "descending", "right_column"):
        assert 0 < info["TilesTraced"] <= info["TilesSelected"], info


def test_ray_counts_are_the_listed_tiles(torch_cuda, base, tdev):
    def rays_of(tiles):
        img = Images(torch_cuda, W, H)
        launch(tdev, torch_cuda, base["cam"], tiles, img)
        return img.words()[2]

    assert rays_of([0, 1, 2, 3, 4]) == ROW0_RAYS
    for tiles in ([7], ALL[0::2], [0, 1, 2, 3, 4], [4, 9, 14, 19]):
        a, b = rays_of(tiles), rays_of(complement(tiles))
        print("rays", tiles, a, b)
        assert a + b == FULL_RAYS, (tiles, a, b)


# ------------------------------------------------- 2. all tiles == rt_trace
def test_every_tile_listed_is_rt_trace(torch_cuda, base, tdev):
    torch = torch_cuda
    img = Images(torch, W, H)
    launch(tdev, torch, base["cam"], ALL[::-1], img)
    tp, tc, tr = img.words()
    info_t = tdev.last_info()
    full = Images(torch, W, H)
    tdev.trace(base["cam"], width=W, height=H, frames=F, max_bounce=B, stream=torch.cuda.current_stream().cuda_stream,
               **full.ptrs())
    fp, fc, fr = full.words()
    info_f = tdev.last_info()
    assert np.array_equal(tp, fp) and np.array_equal(tc, fc) and tr == fr == FULL_RAYS
    assert info_t["TilesSelected"] == info_t["TilesTotal"] == info_f["TilesSelected"] == info_f["TilesTotal"]
    assert (info_t["TilesTraced"], info_t["SegmentsFolded"]) == (info_f["TilesTraced"], info_f["SegmentsFolded"])
    assert info_t["SegmentsFolded"] > 0 and info_t["TilesTraced"] > 0


# ------------------------------------------------- 3. every launch shape and path
SHAPE_LIST = [1, 7, 13, 19]  # live + dead block tiles (1, 13), a live tile, the dead 8 x 8 corner
VARIANTS = [(f"lanes{p}", {"LanesPerPixel": p}, {}) for p in (1, 2, 4, 8, 16, 32)] + [
    ("one_frame_4_pixels_per_lane", {"PixelsPerLane": 4}, {"frames": 1}),
    ("cull_off", {"Cull": OFF}, {}), ("four_wave_groups", {"OneWaveGroups": OFF}, {}),
    ("encode_pass_off", {"EncodePass": OFF}, {}), ("tile_order_off", {"TileOrder": OFF}, {}),
    ("pixel_sort_off", {"PixelSort": OFF}, {}), ("scalar_rules", {}, {"simd": False}),
    ("srgb_pow", {}, {"srgb_pow": True})]


@pytest.mark.parametrize("name,options,how", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_every_launch_shape_and_path(rt, orc, torch_cuda, base, name, options, how):
    frames, simd, srgb_pow = how.get("frames", F), how.get("simd", True), how.get("srgb_pow", False)
    oprev, ocur, _ = base["oracle"](frames, simd)
    if srgb_pow:
        ocur = orc.encode_rgba8(oprev, srgb_pow=True)
    dev = rt.Device(0, options=options)
    try:
        dev.upload_scene(base["s"])
        for launch_no in range(3):  # a new key, the same key again (kept order), and once more (sorted pixels)
            img = Images(torch_cuda, W, H)
            launch(dev, torch_cuda, base["cam"], SHAPE_LIST, img, frames=frames, simd=simd, srgb_pow=srgb_pow)
            assert_tiles(img, SHAPE_LIST, oprev, ocur)
            info = dev.last_info()
            assert info["CullPassRan"] == (1 if launch_no == 0 and name != "cull_off" else 0), info
            assert info["TilesSelected"] == block_tiles(W, H, SHAPE_LIST, info), info
            assert 0 < info["TilesTraced"] <= info["TilesSelected"], info
            if name == "cull_off":
                assert info["TilesTraced"] == info["TilesSelected"] and info["SegmentsFolded"] == 0, info
            else:
                assert info["SegmentsFolded"] > 0, info
            if "LanesPerPixel" in options:
                assert info["LanesPerPixel"] == options["LanesPerPixel"]
            if name.startswith("one_frame"):
                assert info["PixelsPerLane"] == 4
    finally:
        dev.close()


@pytest.mark.parametrize("scene,w,h,frames,full_rays,lists,row0_rays", [
    (2, 72, 40, 2, 12268, ([0, 1, 2], [1, 3, 5]), 11116),  # RTWeekend: sky, no dead tiles
    (0, 96, 72, 4, 53024, ([0, 2, 4, 6, 8],), None),       # RGB Glass: dielectrics, dead bottom tiles
], ids=["rtweekend", "rgb_glass"])
def test_other_scenes(rt, orc, torch_cuda, scene, w, h, frames, full_rays, lists, row0_rays):
    s, o = rt.scene_builtin(scene), orc.scene_builtin(scene)
    cam, ocam = rt.camera_setup(s, w, h), orc.camera(o, w, h)
    oprev, ocur, orays = orc.render(o, ocam, w, h, frames=frames, max_bounce=5)
    assert orays == full_rays
    n = rt.tile_count(w, h)
    dev = rt.Device(0)
    try:
        dev.upload_scene(s)
        for tiles in lists:
            got = []
            for part in (tiles, complement(tiles, n)):
                img = Images(torch_cuda, w, h)
                launch(dev, torch_cuda, cam, part, img, frames=frames, bounces=5)
                got.append(assert_tiles(img, part, oprev, ocur))
                info = dev.last_info()
                assert info["TilesSelected"] == block_tiles(w, h, part, info) and info["TilesTraced"] > 0, info
                if o.use_sky:  # nothing folds under a sky: every selected tile is traced
                    assert info["SegmentsFolded"] == 0 and info["TilesTraced"] == info["TilesSelected"], info
                elif part is tiles:  # RGB Glass: the even tiles hold the dead bottom corners
                    assert info["SegmentsFolded"] > 0, info
            print("rays", scene, tiles, got)
            assert sum(got) == full_rays, (tiles, got)
            if row0_rays is not None and tiles == [0, 1, 2]:
                assert got[0] == row0_rays
    finally:
        dev.close()


# ------------------------------------------------- 4. continuation and the selected-only fold
def test_continuation_and_fold_stay_inside_the_selection(orc, torch_cuda, base, tdev):
    torch = torch_cuda
    mean = np.random.default_rng(44).uniform(0.25, 2.0, (W * H, 4)).astype(np.float32)
    list_a, list_b = [0, 7, 12, 19], [5, 6, 13]  # tile 10 (all dead) is in neither
    o8 = orc.render(base["o"], base["ocam"], W, H, prev_count=3, frames=8, max_bounce=B, prev=mean.copy())
    o4 = orc.render(base["o"], base["ocam"], W, H, prev_count=3, frames=4, max_bounce=B, prev=mean.copy())
    img = Images(torch, W, H, mean=mean)
    launch(tdev, torch, base["cam"], list_a, img, frames=4, prev_count=3)
    launch(tdev, torch, base["cam"], list_b, img, frames=4, prev_count=3)
    info_b = tdev.last_info()
    launch(tdev, torch, base["cam"], list_a, img, frames=4, prev_count=7)
    info_a = tdev.last_info()
    for info in (info_a, info_b):
        assert info["SegmentsFolded"] > 0 and info["TilesTraced"] > 0, info
    gp, gc, _ = img.words()
    ma, mb = tile_mask(W, H, list_a), tile_mask(W, H, list_b)
    for m, (oprev, ocur, _) in ((ma, o8), (mb, o4)):
        assert np.array_equal(gp[m], oprev.view(np.uint32)[m]) and np.array_equal(gc[m], ocur[m])
    rest = ~(ma | mb)
    assert rest[tile_mask(W, H, [10])].all()
    assert np.array_equal(gp[rest], mean.view(np.uint32)[rest]), "a pixel outside both lists was folded"
    assert np.all(gc[rest] == POISON)
    assert np.all(mean[tile_mask(W, H, [10])][:, :3] != 0.0)


# ------------------------------------------------- 5. keys
def test_launch_keys(rt, orc, torch_cuda, base, tdev):
    torch = torch_cuda
    oprev, ocur, _ = base["oracle"]()
    l1, l2 = [7, 13], [2, 6, 19]
    imgs = [Images(torch, W, H) for _ in range(3)]
    for img, tiles in zip(imgs, (l1, l2, l1)):  # back to back: nothing waits for the device in between
        launch(tdev, torch, base["cam"], tiles, img)
    for img, tiles in zip(imgs, (l1, l2, l1)):
        assert_tiles(img, tiles, oprev, ocur)
    ran = []
    for tiles in (l2, l1, l2, l2):  # (the last key above was l1's)
        img = Images(torch, W, H)
        launch(tdev, torch, base["cam"], tiles, img)
        ran.append(tdev.last_info()["CullPassRan"])
        assert_tiles(img, tiles, oprev, ocur)
        info = tdev.last_info()
        assert info["TilesSelected"] == block_tiles(W, H, tiles, info)
    assert ran == [1, 1, 1, 0]
    # a new camera with the same list
    cam2, ocam2 = rt.camera_setup(base["s"], W, H, distance=6.0), orc.camera(base["o"], W, H, distance=6.0)
    o2 = orc.render(base["o"], ocam2, W, H, frames=F, max_bounce=B)
    img = Images(torch, W, H)
    launch(tdev, torch, cam2, l2, img)
    assert tdev.last_info()["CullPassRan"] == 1
    assert_tiles(img, l2, o2[0], o2[1])
    # rt_trace right after a tile launch: no selection survives
    full = Images(torch, W, H)
    tdev.trace(cam2, width=W, height=H, frames=F, max_bounce=B, stream=torch.cuda.current_stream().cuda_stream,
               **full.ptrs())
    fp, fc, fr = full.words()
    assert np.array_equal(fp, o2[0].view(np.uint32)) and np.array_equal(fc, o2[1]) and fr == o2[2]
    info = tdev.last_info()
    assert info["TilesSelected"] == info["TilesTotal"] and info["CullPassRan"] == 1


# ------------------------------------------------- 6. errors
def _raw_call(rt, dev, cam, img, tiles_ptr, n_tiles, *, band_count=1, frames=F):
    c = rt.RtCameraInfo()
    ctypes.pointer(c)[0] = cam
    c.CurrentImage = rt.RtImage(img.cur.data_ptr(), img.w, img.h, rt.RT_FORMAT_R8G8B8A8_U32)
    c.PreviousImage = rt.RtImage(img.prev.data_ptr(), img.w, img.h, rt.RT_FORMAT_R32B32G32A32_F32)
    d = rt.RtTraceDesc(img.w, img.h, 0, frames, B, 1, rt.RT_SEED_PIXEL, 32, band_count, 0, 0)
    return rt.lib().rt_trace_tiles(dev.handle, ctypes.byref(c), ctypes.byref(d), ctypes.c_void_p(tiles_ptr), n_tiles,
                                   ctypes.c_void_p(img.rays.data_ptr()),
                                   ctypes.c_void_p(img.torch.cuda.current_stream().cuda_stream))


def test_argument_errors_enqueue_nothing(rt, torch_cuda, base, tdev):
    img = Images(torch_cuda, W, H)

    def untouched():
        gp, gc, rays = img.words()
        return bool(np.all(gp == POISON) and np.all(gc == POISON) and rays == 0)

    good = np.array([7, 8], np.uint32)
    for what, arr, n, kw in (("an index named twice", np.array([3, 9, 3], np.uint32), 3, {}),
                             ("index 20", np.array([1, 20], np.uint32), 2, {}),
                             ("BandCount 2", good, 2, {"band_count": 2}),
                             ("NULL list", None, 2, {})):
        rc = _raw_call(rt, tdev, base["cam"], img, arr.ctypes.data if arr is not None else None, n, **kw)
        assert rc == -22, (what, rc)
        assert rt.lib().rt_last_error(), what
        assert untouched(), what
    with pytest.raises(rt.RtError):
        launch(tdev, torch_cuda, base["cam"], [4, 4], img)
    assert _raw_call(rt, tdev, base["cam"], img, None, 0) == 0
    assert _raw_call(rt, tdev, base["cam"], img, good.ctypes.data, 0) == 0
    assert _raw_call(rt, tdev, base["cam"], img, good.ctypes.data, 2, frames=0) == 0
    launch(tdev, torch_cuda, base["cam"], [], img)
    assert untouched()


# ------------------------------------------------- 7. host array lifetime
def test_the_list_is_consumed_before_the_call_returns(rt, torch_cuda, base, tdev):
    oprev, ocur, _ = base["oracle"]()
    tiles = [3, 8, 17]  # a list no other test launches on this device: a new key, so the bitmap is uploaded
    arr = np.array(tiles, np.uint32)
    img = Images(torch_cuda, W, H)
    assert _raw_call(rt, tdev, base["cam"], img, arr.ctypes.data, len(arr)) == 0
    arr[:] = 0xFFFFFFFF  # before any sync
    assert tdev.last_info()["CullPassRan"] == 1
    assert_tiles(img, tiles, oprev, ocur)


# ------------------------------------------------- 8. reservation
def test_reserve_covers_tile_launches(rt, torch_cuda, base):
    oprev, ocur, _ = base["oracle"]()
    dev = rt.Device(0)
    try:
        dev.upload_scene(base["s"])
        dev.reserve(W, H)
        growths = dev.last_info()["BufferGrowths"]
        for tiles in LISTS.values():
            img = Images(torch_cuda, W, H)
            launch(dev, torch_cuda, base["cam"], tiles, img)
            assert_tiles(img, tiles, oprev, ocur)
            assert dev.last_info()["BufferGrowths"] == growths
    finally:
        dev.close()


# ------------------------------------------------- 9. a real geometry
def test_windows_of_a_1080p_frame(rt, orc, torch_cuda, base):
    torch = torch_cuda
    w, h = 1920, 1080
    cam, ocam = rt.camera_setup(base["s"], w, h), orc.camera(base["o"], w, h)
    assert rt.tile_count(w, h) == 2040
    dev = rt.Device(0)
    try:
        dev.upload_scene(base["s"])
        # 3 x 3 tiles from (TileX 29, TileY 15), and four tiles of the ragged bottom row (TileY 33: 24 rows)
        for x0, y0, x1, y1, n in ((29 * 32, 15 * 32, 32 * 32, 18 * 32, 9), (28 * 32, 33 * 32, 32 * 32, h, 4)):
            tiles = rt.tiles_of_rect(w, h, x0, y0, x1, y1)
            assert len(tiles) == n and tiles[0] == (y0 // 32) * 60 + x0 // 32
            oprev, ocur, _ = orc.render(base["o"], ocam, w, h, frames=1, max_bounce=B, rows=(y0, y1))
            img = Images(torch, w, h)
            launch(dev, torch, cam, tiles, img, frames=1)
            gp, gc, rays = img.words()
            m = tile_mask(w, h, tiles)
            win = np.zeros((h, w), bool)
            win[y0:y1, x0:x1] = True
            assert np.array_equal(m, win.ravel())
            assert np.array_equal(gp[m], oprev.view(np.uint32)[m]) and np.array_equal(gc[m], ocur[m])
            assert np.all(gp[~m] == POISON) and np.all(gc[~m] == POISON)
            info = dev.last_info()
            assert info["TilesSelected"] == block_tiles(w, h, tiles, info) and info["PixelsPerLane"] == 4, info
            if n == 9:  # the frame's centre sees spheres (the bottom row may hold dead tiles only)
                assert info["TilesTraced"] > 0, info
            assert rays >= int(m.sum())  # every pixel's sample counts a segment, traced or folded
    finally:
        dev.close()
