"""GPU checks of the per-tile RGBA8 change statistics: rt_trace_tile_work_delta (rt_trace_tile_work whose
closing RGBA8 pass also writes, per listed tile, how far the tile's displayed pixels moved) and
rt_tile_delta_rgba8 (the same statistics between two RGBA8 images, nothing traced).  The statistics are
integers without a summation order, so every comparison is bit-exact against a numpy restatement over
the oracle's frames (no tolerance anywhere).

Base input (that of tests/test_gpu_tile_work.py): scene 1 prefix 64, 136 x 104, 8 bounces: TilesX 5,
TilesY 4, the right column 8 px wide, the bottom row 8 px tall, tile 19 8 x 8; the MIXED list."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, B = 136, 104, 8
TILES_X, N_TILES = 5, 20
POISON = 0xDEADBEEF
POISON_I32 = POISON - (1 << 32)
OFF = -1
MEAN = np.random.default_rng(2024).uniform(0.25, 2.0, (W * H, 4)).astype(np.float32)
MEAN.setflags(write=False)
# "old" of a first round: uniformly random bytes, alpha included
OLD = np.random.default_rng(99).integers(0, 1 << 32, W * H, dtype=np.uint64).astype(np.uint32)
OLD.setflags(write=False)
MIXED = {0: (0, 8), 7: (3, 4), 12: (3, 12), 19: (7, 1), 6: (7, 2), 13: (0, 40), 10: (5, 3)}
ROW_PAIRS = [(0, 8), (3, 4), (3, 12), (7, 1)]


def tile_delta_ref(old, new, w, h):
    """(n_tiles, 4) u32 {Changed, MaxDelta, SumDelta, SumSquares} per 32 x 32 tile (clipped) between two
    (h * w,) u32 RGBA8 images; alpha is not looked at."""
    o = old.reshape(h, w).astype(np.uint32)
    n = new.reshape(h, w).astype(np.uint32)
    d = np.stack([np.abs(((o >> s) & 255).astype(np.int64) - ((n >> s) & 255).astype(np.int64)) for s in (0, 8, 16)], -1)
    tx, ty = (w + 31) // 32, (h + 31) // 32
    out = np.zeros((tx * ty, 4), np.uint32)
    for t in range(tx * ty):
        b = d[(t // tx) * 32:(t // tx) * 32 + 32, (t % tx) * 32:(t % tx) * 32 + 32]
        out[t] = (int((b.max(-1) > 0).sum()), int(b.max()), int(b.sum()), int((b * b).sum()))
    return out


def tile_mask(w, h, tiles):
    tx = (w + 31) // 32
    m = np.zeros((h, w), bool)
    for t in tiles:
        m[(t // tx) * 32:(t // tx) * 32 + 32, (t % tx) * 32:(t % tx) * 32 + 32] = True
    return m.ravel()


def triples(work):
    return [(t, p, f) for t, (p, f) in work.items()]


def i32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to("cuda")


class State:
    """Both device images, the ray counter and the statistics array (poisoned) of a sampler."""

    def __init__(self, torch, mean=MEAN, cur=OLD, w=W, h=H):
        self.torch, self.w, self.h, self.n_tiles = torch, w, h, ((w + 31) // 32) * ((h + 31) // 32)
        self.prev = torch.from_numpy(mean.copy()).to("cuda")
        self.cur = i32(torch, cur)
        self.rays = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.delta = torch.full((self.n_tiles * 4,), POISON_I32, dtype=torch.int32, device="cuda")

    def launch(self, dev, cam, work, *, delta=True, srgb_pow=False):
        dev.trace_tile_work(cam, work=triples(work), width=self.w, height=self.h, max_bounce=B, srgb_pow=srgb_pow,
                            stream=self.torch.cuda.current_stream().cuda_stream, prev_ptr=self.prev.data_ptr(),
                            cur_ptr=self.cur.data_ptr(), rays_ptr=self.rays.data_ptr(),
                            delta_ptr=self.delta.data_ptr() if delta else 0)

    def words(self):
        """(mean (h*w, 4) u32, RGBA8 (h*w,) u32, rays, statistics (n_tiles, 4) u32) after a device sync."""
        self.torch.cuda.synchronize()
        return (self.prev.view(self.torch.int32).cpu().numpy().view(np.uint32), self.cur.cpu().numpy().view(np.uint32),
                int(self.rays.item()), self.delta.cpu().numpy().view(np.uint32).reshape(self.n_tiles, 4))


class Oracle:
    """Full-frame oracle renders from one starting mean (default MEAN), one per (PreviousRayCount, Frames)
    pair, cached and read-only."""

    def __init__(self, orc, scene, cam, w=W, h=H, mean=MEAN):
        self.orc, self.scene, self.cam, self.w, self.h, self.mean, self.cache = orc, scene, cam, w, h, mean, {}

    def render(self, pair):
        if pair not in self.cache:
            r = self.orc.render(self.scene, self.cam, self.w, self.h, prev_count=pair[0], frames=pair[1],
                                max_bounce=B, prev=self.mean.copy())
            r[0].setflags(write=False)
            r[1].setflags(write=False)
            self.cache[pair] = r
        return self.cache[pair]

    def expected(self, pairs, base_prev, base_cur, base_delta=None, srgb_pow=False):
        """What a launch leaves: `pairs` {tile: the (PreviousRayCount, Frames) FROM MEAN whose render the tile
        must hold} over the images (base_prev (h*w, 4) u32, base_cur (h*w,) u32) it found; the statistics of
        the listed tiles from (base_cur, new RGBA8), the others as base_delta had them (default: poison)."""
        ep, ec = base_prev.copy(), base_cur.copy()
        for t, pair in pairs.items():
            oprev, ocur, _ = self.render(tuple(pair))
            m = tile_mask(self.w, self.h, [t])
            ep[m] = oprev.view(np.uint32)[m]
            ec[m] = self.orc.encode_rgba8(oprev[m], srgb_pow=True) if srgb_pow else ocur[m]
        n_tiles = ((self.w + 31) // 32) * ((self.h + 31) // 32)
        ed = np.full((n_tiles, 4), POISON, np.uint32) if base_delta is None else base_delta.copy()
        ref = tile_delta_ref(base_cur, ec, self.w, self.h)
        for t in pairs:
            ed[t] = ref[t]
        return ep, ec, ed


def assert_state(st, exp, what=""):
    ep, ec, ed = exp
    gp, gc, rays, gd = st.words()
    bad = np.flatnonzero((gp != ep).any(1))
    assert bad.size == 0, f"{what}: {bad.size} pixels' means differ, first pixel {bad[0]}"
    badc = np.flatnonzero(gc != ec)
    assert badc.size == 0, f"{what}: {badc.size} RGBA8 pixels differ, first pixel {badc[0]}"
    print(what, "statistics", {t: gd[t].tolist() for t in range(len(gd)) if not np.all(gd[t] == POISON)})
    badd = np.flatnonzero((gd != ed).any(1))
    assert badd.size == 0, f"{what}: tiles {badd.tolist()}: got {gd[badd].tolist()}, expected {ed[badd].tolist()}"
    return rays


def distinct_and_non_zero(ed, tiles):
    rows = [tuple(int(v) for v in ed[t]) for t in tiles]
    return len(set(rows)) == len(rows) and all(all(v > 0 for v in r) for r in rows)


@pytest.fixture(scope="module")
def base(rt, orc, torch_cuda):
    s, o = rt.scene_prefix(rt.scene_builtin(1), 64), orc.scene_builtin(1).prefix(64)
    cam, ocam = rt.camera_setup(s, W, H), orc.camera(o, W, H)
    return dict(s=s, o=o, cam=cam, ocam=ocam, oracle=Oracle(orc, o, ocam))


@pytest.fixture(scope="module")
def tdev(rt, torch_cuda, base):
    dev = rt.Device(0)
    dev.upload_scene(base["s"])
    yield dev
    dev.close()


def plain_rays(torch, dev, cam, work, srgb_pow=False):
    """The ray count of rt_trace_tile_work itself over `work` (from MEAN, on the same device and key)."""
    st = State(torch)
    st.launch(dev, cam, work, delta=False, srgb_pow=srgb_pow)
    return st.words()[2]


# ------------------------------------------------- 1 + 2. mixed pairs from random bytes, then a realistic round
def test_mixed_pairs_then_a_doubling_round(torch_cuda, base, tdev):
    oracle, mean_u = base["oracle"], MEAN.view(np.uint32)
    exp1 = oracle.expected(MIXED, mean_u, OLD)
    # a swapped or dropped tile cannot pass: the expected entries differ pairwise and hold no zero
    assert distinct_and_non_zero(exp1[2], list(MIXED)), exp1[2][list(MIXED)].tolist()
    st = State(torch_cuda)
    st.launch(tdev, base["cam"], MIXED)
    rays1 = assert_state(st, exp1, "round 1")
    info = tdev.last_info()
    assert info["TileCounts"] == 1 and info["SplitHeadFrames"] == 0 and info["LanesPerPixel"] == 16, info
    assert 0 < info["TilesTraced"] < info["TilesSelected"] and info["SegmentsFolded"] > 0, info  # (dead tiles too)
    assert rays1 == plain_rays(torch_cuda, tdev, base["cam"], MIXED) > 0
    # round 2: every tile doubles its sample count; "old" is what round 1 stored, nothing is re-poisoned
    work2 = {t: (p + f, p + f) for t, (p, f) in MIXED.items()}
    exp2 = oracle.expected({t: (p, p + 2 * f) for t, (p, f) in MIXED.items()}, exp1[0], exp1[1], exp1[2])
    listed = exp2[2][list(MIXED)]
    assert int((listed[:, 0] > 0).sum()) >= 3 and len(set(listed[:, 1].tolist())) > 1, listed.tolist()
    st.launch(tdev, base["cam"], work2)
    rays2 = assert_state(st, exp2, "round 2") - rays1
    assert tdev.last_info()["CullPassRan"] == 0  # (the counts and the statistics are no part of the key)
    st2 = State(torch_cuda, mean=exp1[0].view(np.float32), cur=exp1[1])
    st2.launch(tdev, base["cam"], work2, delta=False)
    assert rays2 == st2.words()[2] > 0


def test_ray_count_is_the_oracles(orc, torch_cuda, base, tdev):
    """Every tile listed, a pair per tile row: the oracle counts rows, so the ray count is checked against it alone."""
    work = {t: ROW_PAIRS[t // TILES_X] for t in range(N_TILES)}
    st = State(torch_cuda)
    st.launch(tdev, base["cam"], work)
    rays = assert_state(st, base["oracle"].expected(work, MEAN.view(np.uint32), OLD), "rows")
    want = sum(orc.render(base["o"], base["ocam"], W, H, prev_count=p, frames=f, max_bounce=B, prev=MEAN.copy(),
                          rows=(32 * r, min(H, 32 * r + 32)))[2] for r, (p, f) in enumerate(ROW_PAIRS))
    assert rays == want


# ------------------------------------------------- 3. uniform pairs
@pytest.mark.parametrize("pair,options", [((5, 1), {}), ((3, 40), {"HeadSamples": 1, "LanesPerPixel": 8})],
                         ids=["one_frame_4_pixels_per_lane", "split_first_launch"])
def test_uniform_pair(rt, torch_cuda, base, pair, options):
    tiles = [1, 7, 13, 19]
    work = {t: pair for t in tiles}
    exp = base["oracle"].expected(work, MEAN.view(np.uint32), OLD)
    assert distinct_and_non_zero(exp[2], tiles)
    dev = rt.Device(0, options=options)
    try:
        dev.upload_scene(base["s"])
        st = State(torch_cuda)
        st.launch(dev, base["cam"], work)
        rays = assert_state(st, exp, str(pair))
        info = dev.last_info()
        assert info["TileCounts"] == 0 and info["CullPassRan"] == 1, info  # (rt_trace_last_tile_counts is 0)
        if pair[1] == 1:  # the shape whose trace kernel would otherwise store RGBA8 itself
            assert info["PixelsPerLane"] == 4 and info["LanesPerPixel"] == 1 and info["SplitHeadFrames"] == 0, info
        else:
            assert info["SplitHeadFrames"] > 0, info
        assert rays == plain_rays(torch_cuda, dev, base["cam"], work) > 0
    finally:
        dev.close()


# ------------------------------------------------- 4 + 5. options and the pow curve
@pytest.mark.parametrize("options,srgb_pow", [({"EncodePass": OFF}, False), ({"OneWaveGroups": OFF}, False), ({}, True)],
                         ids=["encode_pass_off", "four_wave_groups", "srgb_pow"])
def test_options_and_srgb_pow(rt, torch_cuda, base, options, srgb_pow):
    exp = base["oracle"].expected(MIXED, MEAN.view(np.uint32), OLD, srgb_pow=srgb_pow)
    assert distinct_and_non_zero(exp[2], list(MIXED))
    if srgb_pow:  # "new" is the pow curve's bytes, and they are not the sqrt curve's
        assert not np.array_equal(exp[1], base["oracle"].expected(MIXED, MEAN.view(np.uint32), OLD)[1])
    dev = rt.Device(0, options=options)
    try:
        dev.upload_scene(base["s"])
        st = State(torch_cuda)
        st.launch(dev, base["cam"], MIXED, srgb_pow=srgb_pow)
        rays = assert_state(st, exp, str(options))
        info = dev.last_info()
        assert info["TileCounts"] == 1 and info["OneWaveGroups"] == (0 if "OneWaveGroups" in options else 1), info
        assert rays == plain_rays(torch_cuda, dev, base["cam"], MIXED, srgb_pow) > 0
    finally:
        dev.close()


# ------------------------------------------------- a width off the 4-pixel grid: the pass's dword path
def test_odd_width(rt, orc, torch_cuda):
    """70 x 40: TilesX 3, TilesY 2, the right column 6 px wide (a lane's four pixels cross the image edge), the
    bottom row 8 px tall; RGBA8 rows are 280 bytes, so every other row starts off the 16-byte grid."""
    w, h = 70, 40
    s, o = rt.scene_prefix(rt.scene_builtin(1), 64), orc.scene_builtin(1).prefix(64)
    cam, ocam = rt.camera_setup(s, w, h), orc.camera(o, w, h)
    rng = np.random.default_rng(11)
    mean = rng.uniform(0.25, 2.0, (w * h, 4)).astype(np.float32)
    old = rng.integers(0, 1 << 32, w * h, dtype=np.uint64).astype(np.uint32)
    work = {0: (0, 4), 2: (3, 2), 4: (2, 5), 5: (7, 1)}  # (tile 1 and tile 3 stay untouched)
    exp = Oracle(orc, o, ocam, w, h, mean).expected(work, mean.view(np.uint32), old)
    assert distinct_and_non_zero(exp[2], list(work))
    dev = rt.Device(0)
    try:
        dev.upload_scene(s)
        st = State(torch_cuda, mean, old, w, h)
        st.launch(dev, cam, work)
        assert assert_state(st, exp, "70 x 40") > 0
        assert dev.last_info()["TileCounts"] == 1
    finally:
        dev.close()


# ------------------------------------------------- 6. the launch key
def test_the_statistics_are_not_in_the_key(rt, torch_cuda, base):
    dev = rt.Device(0)
    try:
        dev.upload_scene(base["s"])
        st = State(torch_cuda)
        st.launch(dev, base["cam"], MIXED, delta=False)
        assert dev.last_info()["CullPassRan"] == 1
        assert np.all(st.words()[3] == POISON)  # (the plain call writes no statistics)
        st = State(torch_cuda)
        st.launch(dev, base["cam"], MIXED)
        assert_state(st, base["oracle"].expected(MIXED, MEAN.view(np.uint32), OLD), "second call")
        assert dev.last_info()["CullPassRan"] == 0
    finally:
        dev.close()


# ------------------------------------------------- 7. zero-frame entries and empty lists
def test_zero_frame_entries_and_empty_lists(torch_cuda, base, tdev):
    work = {0: (0, 8), 5: (4, 0), 7: (3, 4), 8: (0, 0), 19: (7, 1), 10: (0xFFFFFFFF, 0)}
    kept = {t: p for t, p in work.items() if p[1]}
    st = State(torch_cuda)
    st.launch(tdev, base["cam"], work)
    assert_state(st, base["oracle"].expected(kept, MEAN.view(np.uint32), OLD), "zero frames")  # (5, 8, 10: untouched)
    for what, empty in (("all zero", {3: (0, 0), 4: (9, 0)}), ("empty", {})):
        st = State(torch_cuda)
        st.launch(tdev, base["cam"], empty)
        gp, gc, rays, gd = st.words()
        assert np.array_equal(gp, MEAN.view(np.uint32)) and np.array_equal(gc, OLD) and rays == 0, what
        assert np.all(gd == POISON), what


# ------------------------------------------------- 8. rt_tile_delta_rgba8
def delta_of(rt, torch, old, new, w, h, *, offset=0):
    """rt_tile_delta_rgba8 over two host images; offset: elements the device images start past their buffers."""
    n = ((w + 31) // 32) * ((h + 31) // 32)
    pad = np.zeros(offset, np.uint32)
    d_old, d_new = i32(torch, np.concatenate([pad, old]))[offset:], i32(torch, np.concatenate([pad, new]))[offset:]
    out = torch.full((n * 4,), POISON_I32, dtype=torch.int32, device="cuda")
    assert d_old.data_ptr() % 16 == (4 * offset) % 16
    rt.tile_delta_rgba8(d_old.data_ptr(), d_new.data_ptr(), w, h, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_old.cpu().numpy().view(np.uint32), old) and np.array_equal(
        d_new.cpu().numpy().view(np.uint32), new)  # (nothing but the statistics is written)
    return out.cpu().numpy().view(np.uint32).reshape(n, 4)


def test_tile_delta_rgba8(rt, torch_cuda):
    rng = np.random.default_rng(5)

    def rand(n):
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)

    # 67 x 33: a width not divisible by 4, the last column 3 px wide, the last row 1 px tall
    a, b = rand(67 * 33), rand(67 * 33)
    got = delta_of(rt, torch_cuda, a, b, 67, 33)
    assert got.shape == (6, 4) and np.array_equal(got, tile_delta_ref(a, b, 67, 33)), got.tolist()
    n = 64 * 64
    zero = np.zeros(n, np.uint32)
    got = delta_of(rt, torch_cuda, zero, np.full(n, 0x00FFFFFF, np.uint32), 64, 64)
    assert (got == [1024, 255, 783360, 199756800]).all(), got.tolist()
    got = delta_of(rt, torch_cuda, zero, np.full(n, 0xFF000000, np.uint32), 64, 64)  # alpha is not looked at
    assert (got == 0).all(), got.tolist()
    # one G byte off by one, in the last pixel of the last lane of tile 1 (row 31, column 63)
    a = rand(n)
    b = a.copy()
    b[31 * 64 + 63] ^= 0x00000100
    assert delta_of(rt, torch_cuda, a, b, 64, 64).tolist() == [[0] * 4, [1] * 4, [0] * 4, [0] * 4]
    # an image base off the 16-byte grid at a width divisible by 4: the dword path, the same numbers
    a, b = rand(n), rand(n)
    want = tile_delta_ref(a, b, 64, 64)
    assert np.array_equal(delta_of(rt, torch_cuda, a, b, 64, 64), want)
    assert np.array_equal(delta_of(rt, torch_cuda, a, b, 64, 64, offset=1), want)
