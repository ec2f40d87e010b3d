"""GPU checks of rt_trace_tile_counts and of the loop it closes with rt_tile_counts_step: a launch over a host
list of the reference's 32 x 32 tiles in which every tile takes its (PreviousRayCount, Frames) pair from a table in
DEVICE memory when the launch runs, and a tile whose pair folds no frame rests -- no byte of either image, no
d_delta entry, no ray.  Every pixel of a tile that folds a frame gets exactly the bits of the full-frame
`oracle.render` at its pair; the list alone is the launch key; the host never reads the table.  Every comparison
is bit-exact.  Tables are written to the device as torch tensors.

Base input and helpers: those of tests/test_gpu_tile_work.py (scene 1 prefix 64, 136 x 104, 8 bounces, a random
starting mean, poisoned RGBA8; tiles 0, 5, 10, 14, 15 and 19 hold dead block tiles only, tiles 1-3, 6-8 and 11-13
mix live and dead ones; the right column, the bottom row and the corner are clipped)."""
import ctypes

import numpy as np
import pytest

from test_gpu_tile_delta import tile_delta_ref
from test_gpu_tile_work import (B, H, MEAN, MIXED, N_TILES, OFF, POISON, SET_2, W, Images, Oracle, assert_work,
                                base, block_tiles, tile_mask, triples)  # noqa: F401  (base: the module's fixture)

pytestmark = pytest.mark.gpu

U32 = 0xFFFFFFFF
# case 1: MIXED's seven tiles fold their pairs; tile 3 (mixed: live and dead block tiles) and tile 14 (dead only)
# are listed and rest -- tile 14 at PreviousRayCount 0, where a dead block tile folded "by its pair" would store a
# zero mean; unlisted tiles 1, 2, 8, 11 and 16 hold garbage with Frames > 0, which nothing may read
LIST_1 = [0, 6, 7, 10, 12, 13, 19, 3, 14]
TABLE_1 = {**MIXED, 3: (5, 0), 14: (0, 0), 1: (123, 7), 2: (U32, 5), 8: (0, 40), 11: (U32 - 1, U32), 16: (9, 9)}
MAX_1 = 40


def device_table(torch, entries, n=N_TILES):
    """(n, 2) int32 device tensor of rt_tile_counts entries: `entries` {tile: (prev, frames)}, {0, 0} elsewhere."""
    t = np.zeros((n, 2), np.uint32)
    for tile, pair in entries.items():
        t[tile] = pair
    return torch.from_numpy(t.view(np.int32)).to("cuda")


def poisoned_delta(torch, n=N_TILES):
    return torch.full((n * 4,), POISON - (1 << 32), dtype=torch.int32, device="cuda")


def launch(dev, torch, cam, tiles, table, max_frames, img, delta=None, *, bounces=B, simd=True, srgb_pow=False):
    dev.trace_tile_counts(cam, tiles=tiles, counts_ptr=table.data_ptr(), max_frames=max_frames, width=img.w,
                          height=img.h, delta_ptr=delta.data_ptr() if delta is not None else 0, max_bounce=bounces,
                          simd=simd, srgb_pow=srgb_pow, stream=torch.cuda.current_stream().cuda_stream, **img.ptrs())


def active(tiles, entries, max_frames):
    """{tile: (prev, effective frames)} of the listed tiles that fold a frame (the header's clamp)."""
    out = {}
    for t in tiles:
        p, f = entries.get(t, (0, 0))
        f = min(f, max_frames)
        if f and p + f <= U32:
            out[t] = (p, f)
    return out


def assert_delta(delta, work, old_cur, new_cur, w=W, h=H, what=""):
    """d_delta entries of the tiles in `work` are the statistics between old_cur and new_cur; all others are poison."""
    got = delta.cpu().numpy().view(np.uint32).reshape(-1, 4)
    ref = tile_delta_ref(old_cur, new_cur, w, h)
    for t in range(got.shape[0]):
        if t in work:
            assert got[t].tolist() == ref[t].tolist(), (what, t, got[t].tolist(), ref[t].tolist())
        else:
            assert (got[t] == POISON).all(), (what, "entry written", t, got[t].tolist())


@pytest.fixture(scope="module")
def cdev(rt, torch_cuda, base):
    dev = rt.Device(0)
    dev.upload_scene(base["s"])
    yield dev
    dev.close()


# ------------------------------------------------- 1. parity and untouched bytes
def test_parity_and_untouched_bytes(rt, torch_cuda, base):
    dev = rt.Device(0)
    try:
        dev.upload_scene(base["s"])
        img, delta = Images(torch_cuda), poisoned_delta(torch_cuda)
        launch(dev, torch_cuda, base["cam"], LIST_1, device_table(torch_cuda, TABLE_1), MAX_1, img, delta)
        assert active(LIST_1, TABLE_1, MAX_1) == MIXED
        exp = base["oracle"].expected(MIXED)
        # (every other word of both images is what it was, the resting tiles 3 and 14 included)
        assert_work(img, exp, "device table")
        assert_delta(delta, MIXED, np.full(W * H, POISON, np.uint32), exp[1], what="case 1")
        info = dev.last_info()
        assert info["TileCounts"] == 1 and info["SplitHeadFrames"] == 0 and info["CullPassRan"] == 1, info
        assert info["TilesSelected"] == block_tiles(W, H, LIST_1, info), info  # (all nine: the list is the key)
        assert info["LanesPerPixel"] == 16 and info["SegmentsFolded"] > 0, info
    finally:
        dev.close()


# ------------------------------------------------- 2. the same as the host-driven call
def test_same_as_the_host_driven_call(rt, torch_cuda, base):
    got = []
    for device_side in (True, False):  # a fresh device each: both calls are their key's first launch
        dev = rt.Device(0)
        try:
            dev.upload_scene(base["s"])
            img, delta = Images(torch_cuda), poisoned_delta(torch_cuda)
            if device_side:
                launch(dev, torch_cuda, base["cam"], LIST_1, device_table(torch_cuda, TABLE_1), MAX_1, img, delta)
            else:
                dev.trace_tile_work(base["cam"], work=triples({t: TABLE_1[t] for t in LIST_1}), width=W, height=H,
                                    max_bounce=B, delta_ptr=delta.data_ptr(),
                                    stream=torch_cuda.cuda.current_stream().cuda_stream, **img.ptrs())
            gp, gc, rays = img.words()
            got.append((gp, gc, rays, dev.last_info()["SegmentsFolded"],
                        delta.cpu().numpy().view(np.uint32).reshape(-1, 4)))
        finally:
            dev.close()
    (ap, ac, ar, af, ad), (bp, bc, br, bf, bd) = got
    assert np.array_equal(ap, bp) and np.array_equal(ac, bc)
    print("rays", ar, br, "SegmentsFolded", af, bf)
    assert ar == br and ar > 0 and af == bf and af > 0
    assert np.array_equal(ad[sorted(MIXED)], bd[sorted(MIXED)])
    assert np.array_equal(ad, bd)  # (and the poison of every other entry)


# ------------------------------------------------- 3. every launch shape and path
# a mixed tile with live blocks (1), a live tile (7), a mixed tile (13), the dead corner (19); resting: the mixed
# tile 3 (live and dead blocks) and the dead tile 14
SHAPE_LIST = [1, 7, 3, 13, 14, 19]
SHAPE_TABLE = {1: (0, 8), 7: (3, 4), 13: (3, 12), 19: (7, 1), 3: (2, 0), 14: (0, 0), 8: (1, 1)}
ONE_FRAME_TABLE = {1: (0, 1), 7: (3, 1), 13: (5, 1), 19: (7, 1), 3: (2, 0), 14: (0, 0), 8: (1, 1)}
VARIANTS = [(f"lanes{p}", {"LanesPerPixel": p}, {}) for p in (1, 2, 4, 8, 16, 32)] + [
    ("max_frames_1", {}, {"table": ONE_FRAME_TABLE, "max_frames": 1}),
    ("four_wave_groups", {"OneWaveGroups": OFF}, {}),
    ("four_wave_scene_in_hbm", {"OneWaveGroups": OFF, "SceneInHbm": 1}, {"routed": True}),
    ("scalar_rules", {}, {"simd": False}), ("srgb_pow", {}, {"srgb_pow": True}),
    ("encode_pass_off", {"EncodePass": OFF}, {}), ("cull_off", {"Cull": OFF}, {})]


@pytest.mark.parametrize("name,options,how", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_every_launch_shape_and_path(rt, torch_cuda, base, name, options, how):
    table, max_frames = how.get("table", SHAPE_TABLE), how.get("max_frames", 12)
    simd, srgb_pow = how.get("simd", True), how.get("srgb_pow", False)
    work = active(SHAPE_LIST, table, max_frames)
    assert sorted(work) == [1, 7, 13, 19]
    exp = base["oracle"].expected(work, simd, srgb_pow)
    d_table = device_table(torch_cuda, table)
    dev = rt.Device(0, options=options)
    try:
        dev.upload_scene(base["s"])
        # a new key, the same key again (the order re-sorted from costs the resting units took part in), and once
        # more (sorted pixels); the middle launch without statistics: RGBA8 as rt_trace_tile_work stores it
        for launch_no in range(3):
            img = Images(torch_cuda)
            delta = poisoned_delta(torch_cuda) if launch_no != 1 else None
            launch(dev, torch_cuda, base["cam"], SHAPE_LIST, d_table, max_frames, img, delta, simd=simd, srgb_pow=srgb_pow)
            assert_work(img, exp, f"{name} launch {launch_no}")
            if delta is not None:
                assert_delta(delta, work, np.full(W * H, POISON, np.uint32), exp[1], what=name)
            info = dev.last_info()
            assert info["TileCounts"] == 1 and info["SplitHeadFrames"] == 0, info
            assert info["CullPassRan"] == (1 if launch_no == 0 and name != "cull_off" else 0), info
            assert info["TilesSelected"] == block_tiles(W, H, SHAPE_LIST, info), info
            if name == "cull_off":
                assert info["TilesTraced"] == info["TilesSelected"] and info["SegmentsFolded"] == 0, info
            else:
                assert 0 < info["TilesTraced"] < info["TilesSelected"] and info["SegmentsFolded"] > 0, info
            if "LanesPerPixel" in options:
                assert info["LanesPerPixel"] == options["LanesPerPixel"]
            if name == "max_frames_1":
                assert info["PixelsPerLane"] == 4 and info["LanesPerPixel"] == 1, info
            if name == "four_wave_groups":
                assert info["OneWaveGroups"] == 0, info
            if how.get("routed"):
                assert info["OneWaveGroups"] == 1 and info["Walk"] == 0, info
    finally:
        dev.close()


def test_rtweekend_one_tile_rests(rt, orc, torch_cuda):
    """RTWeekend at 72 x 40 has sky: nothing is dead, nothing folds; tile 3 of the six rests."""
    w, h = 72, 40
    s, o = rt.scene_builtin(2), orc.scene_builtin(2)
    cam, ocam = rt.camera_setup(s, w, h), orc.camera(o, w, h)
    mean = np.random.default_rng(7).uniform(0.25, 2.0, (w * h, 4)).astype(np.float32)
    table = {0: (0, 2), 1: (2, 3), 2: (0, 2), 3: (2, 0), 4: (2, 3), 5: (2, 3)}
    work = active(range(6), table, 3)
    assert sorted(work) == [0, 1, 2, 4, 5]
    exp = Oracle(orc, o, ocam, w, h, mean, 5).expected(work)
    dev = rt.Device(0)
    try:
        dev.upload_scene(s)
        for launch_no in range(2):
            img, delta = Images(torch_cuda, w, h, mean), poisoned_delta(torch_cuda, 6)
            launch(dev, torch_cuda, cam, list(range(6)), device_table(torch_cuda, table, 6), 3, img, delta, bounces=5)
            assert_work(img, exp, f"rtweekend launch {launch_no}")
            assert_delta(delta, work, np.full(w * h, POISON, np.uint32), exp[1], w, h, "rtweekend")
            info = dev.last_info()
            assert info["TileCounts"] == 1 and info["SegmentsFolded"] == 0, info
            assert info["TilesTraced"] == info["TilesSelected"] == info["TilesTotal"], info
    finally:
        dev.close()


# ------------------------------------------------- 4. clamps
def test_clamps(torch_cuda, base, cdev):
    # Frames = 100 under max_frames = 12: the bits of (prev, 12)
    img, delta = Images(torch_cuda), poisoned_delta(torch_cuda)
    table = {7: (3, 100), 6: (7, 2)}
    launch(cdev, torch_cuda, base["cam"], [7, 6], device_table(torch_cuda, table), 12, img, delta)
    exp = base["oracle"].expected({7: (3, 12), 6: (7, 2)})
    assert_work(img, exp, "Frames above max_frames")
    assert_delta(delta, {7, 6}, np.full(W * H, POISON, np.uint32), exp[1], what="clamp")
    # {0xFFFFFFF0, 0x20} under max_frames = 0x20 does not fit a u32: that tile writes nothing (tile 7 beside it does)
    img, delta = Images(torch_cuda), poisoned_delta(torch_cuda)
    table = {12: (0xFFFFFFF0, 0x20), 7: (3, 12)}
    launch(cdev, torch_cuda, base["cam"], [12, 7], device_table(torch_cuda, table), 0x20, img, delta)
    exp = base["oracle"].expected({7: (3, 12)})
    assert_work(img, exp, "an entry past u32")
    assert_delta(delta, {7}, np.full(W * H, POISON, np.uint32), exp[1], what="past u32")
    # and alone: nothing at all
    img, delta = Images(torch_cuda), poisoned_delta(torch_cuda)
    launch(cdev, torch_cuda, base["cam"], [12], device_table(torch_cuda, {12: (0xFFFFFFF0, 0x20)}), 0x20, img, delta)
    gp, gc, rays = img.words()
    assert np.array_equal(gp, MEAN.view(np.uint32)) and np.all(gc == POISON) and rays == 0
    assert_delta(delta, {}, gc, gc, what="alone")


# ------------------------------------------------- 5. the key, and waking
# round 2: tile 3 wakes, tile 7 rests at its new count, the others go on from theirs (SET_2 continues MIXED);
# round 3: tile 7 and the dead tile 14 wake, tile 19 rests
ROUND_2 = {**{t: SET_2[t] for t in SET_2 if t != 7}, 3: (0, 4), 7: (7, 0), 14: (0, 0)}
ROUND_3 = {0: (10, 6), 6: (10, 3), 7: (7, 5), 10: (16, 1), 12: (18, 7), 13: (60, 4), 19: (13, 0), 3: (4, 3), 14: (0, 2)}


def continued(orc, base, mean_words, cur, work):
    """Expected (mean words, RGBA8, mask) of a launch over `work` on images that hold mean_words / cur."""
    mean = mean_words.view(np.float32).copy()
    ep, ec, listed = Oracle(orc, base["o"], base["ocam"], W, H, mean, B).expected(work)
    return ep, np.where(listed, ec, cur), listed


def test_key_and_waking(rt, orc, torch_cuda, base):
    for t in SET_2:
        assert SET_2[t][0] == MIXED[t][0] + MIXED[t][1]  # (SET_2 continues MIXED)
    dev = rt.Device(0)
    try:
        dev.upload_scene(base["s"])
        dev.reserve(W, H)  # (case 7: BufferGrowths constant over these calls)
        growths = dev.last_info()["BufferGrowths"]
        img, delta = Images(torch_cuda), poisoned_delta(torch_cuda)
        table = device_table(torch_cuda, TABLE_1)
        next_tables = [device_table(torch_cuda, ROUND_2), device_table(torch_cuda, ROUND_3)]  # (uploaded beforehand)
        launch(dev, torch_cuda, base["cam"], LIST_1, table, MAX_1, img, delta)
        info1 = dev.last_info()
        # the table rewritten on the device, in stream order, and the next call: no synchronisation in between
        table.copy_(next_tables[0], non_blocking=True)
        launch(dev, torch_cuda, base["cam"], LIST_1, table, MAX_1, img, delta)
        info2 = dev.last_info()
        e1 = base["oracle"].expected(MIXED)
        work2 = active(LIST_1, ROUND_2, MAX_1)
        assert sorted(work2) == [0, 3, 6, 10, 12, 13, 19]
        e2 = continued(orc, base, e1[0], e1[1], work2)
        assert_work(img, e2, "round 2")
        # (tile 7's entry is round 1's: not written again)
        got = delta.cpu().numpy().view(np.uint32).reshape(-1, 4)
        ref1 = tile_delta_ref(np.full(W * H, POISON, np.uint32), e1[1], W, H)
        ref2 = tile_delta_ref(e1[1], e2[1], W, H)
        for t in range(N_TILES):
            want = ref2[t] if t in work2 else ref1[t] if t == 7 else np.full(4, POISON, np.uint32)
            assert got[t].tolist() == want.tolist(), ("round 2 delta", t)
        table.copy_(next_tables[1], non_blocking=True)
        launch(dev, torch_cuda, base["cam"], LIST_1, table, MAX_1, img, delta)
        info3 = dev.last_info()
        work3 = active(LIST_1, ROUND_3, MAX_1)
        assert sorted(work3) == [0, 3, 6, 7, 10, 12, 13, 14]
        assert_work(img, continued(orc, base, e2[0], e2[1], work3), "round 3")
        print([(i["CullPassRan"], i["OrderedLaunches"], i["PixelsSorted"]) for i in (info1, info2, info3)])
        assert [i["CullPassRan"] for i in (info1, info2, info3)] == [1, 0, 0]
        assert info1["OrderedLaunches"] < info2["OrderedLaunches"] < info3["OrderedLaunches"]
        assert all(i["TileCounts"] == 1 and i["BufferGrowths"] == growths for i in (info1, info2, info3))
        assert len({(i["TilesSelected"], i["TilesTraced"]) for i in (info1, info2, info3)}) == 1
        # a mixed rt_trace_tile_work call over the same nine tiles: the same key (largest Frames 12: 16 lanes per
        # pixel again -- the launch shape is part of every key)
        img = Images(torch_cuda)
        work = {t: (3, 10 + t % 3) for t in LIST_1}
        dev.trace_tile_work(base["cam"], work=triples(work), width=W, height=H, max_bounce=B,
                            stream=torch_cuda.cuda.current_stream().cuda_stream, **img.ptrs())
        assert_work(img, base["oracle"].expected(work), "rt_trace_tile_work over the list")
        info = dev.last_info()
        assert info["CullPassRan"] == 0 and info["TileCounts"] == 1 and info["BufferGrowths"] == growths, info
    finally:
        dev.close()


# ------------------------------------------------- 6. all resting
def test_all_resting_writes_nothing(rt, torch_cuda, base):
    resting = {t: (t, 0) for t in LIST_1}
    resting[12] = (0xFFFFFFF0, 0x20)  # (and one that cannot fold)
    dev = rt.Device(0)
    try:
        dev.upload_scene(base["s"])
        for launch_no in range(3):  # a new key (the cull pass still runs), the key again, and after a re-sort
            img, delta = Images(torch_cuda), poisoned_delta(torch_cuda)
            launch(dev, torch_cuda, base["cam"], LIST_1, device_table(torch_cuda, resting), 0x20, img, delta)
            gp, gc, rays = img.words()
            assert np.array_equal(gp, MEAN.view(np.uint32)) and np.all(gc == POISON) and rays == 0, launch_no
            assert np.all(delta.cpu().numpy().view(np.uint32) == POISON), launch_no
            info = dev.last_info()
            assert info["SegmentsFolded"] == 0 and info["TileCounts"] == 1, info
            assert info["CullPassRan"] == (1 if launch_no == 0 else 0), info
        # the list still traces once its tiles wake (the order kept every live unit in its prefix); under this
        # key's max_frames tile 13's 40 frames are 32
        img, delta = Images(torch_cuda), poisoned_delta(torch_cuda)
        launch(dev, torch_cuda, base["cam"], LIST_1, device_table(torch_cuda, TABLE_1), 0x20, img, delta)
        awake = active(LIST_1, TABLE_1, 0x20)
        assert awake == {**MIXED, 13: (0, 32)}
        assert_work(img, base["oracle"].expected(awake), "awake")
        assert dev.last_info()["CullPassRan"] == 0
    finally:
        dev.close()


# ------------------------------------------------- 7. reservation (with case 5's calls: test_key_and_waking)
def test_reserve_covers_the_call(rt, torch_cuda, base):
    dev = rt.Device(0)
    try:
        dev.upload_scene(base["s"])
        dev.reserve(W, H)
        growths = dev.last_info()["BufferGrowths"]
        for tiles, table, max_frames in ((LIST_1, TABLE_1, MAX_1), (SHAPE_LIST, SHAPE_TABLE, 12),
                                         (SHAPE_LIST, ONE_FRAME_TABLE, 1), (list(range(N_TILES)), TABLE_1, 3)):
            img, delta = Images(torch_cuda), poisoned_delta(torch_cuda)
            launch(dev, torch_cuda, base["cam"], tiles, device_table(torch_cuda, table), max_frames, img, delta)
            assert_work(img, base["oracle"].expected(active(tiles, table, max_frames)), str(tiles))
            info = dev.last_info()
            assert info["BufferGrowths"] == growths and info["TileCounts"] == 1, info
    finally:
        dev.close()


# ------------------------------------------------- 8. the closed loop
# INTEGRATION.md Level 2d as written: for round: rt_trace_tile_counts; rt_tile_counts_step; one asynchronous 16-byte
# summary copy per round -- against Level 2c's loop driven from the host with the rule restated in numpy.
# FIRST 2, doubling, at most 16 a round and 32 a tile: rounds fold 2, 2, 4, 8, 16 frames, round 6 finds every tile
# at rest.  REST_MAX_DELTA 2 at 8 bounces: on the oracle alone (oracle.render per pair, statistics in numpy, checked
# on the CPU before the case went to a GPU) round 2 moves no byte of tiles 0, 5, 9, 10, 14-19 (the dead tiles, and
# tiles whose few lit pixels show only at more samples) and tile 13's bytes by 2 at most, so these eleven rest after
# their second round; the other nine move by 38 to 255 in every later round and are traced through round 5.
ROUNDS, FIRST, MAX_ROUND, MAX_TILE, REST_MAX_DELTA = 6, 2, 16, 32, 2


def rule_numpy(counts, delta):
    """rt_tile_counts_step restated (the rule of tests/test_tile_counts_step.py, at this case's constants)."""
    out, summary = counts.copy(), [0, 0, 0]
    for t in range(counts.shape[0]):
        prev, frames = int(counts[t, 0]), int(counts[t, 1])
        f = min(frames, MAX_ROUND)
        if f == 0 or prev + f > U32:
            continue
        done = prev + f
        rest = done >= MAX_TILE or (prev != 0 and int(delta[t, 1]) <= REST_MAX_DELTA)
        nxt = 0 if rest else min(done, MAX_ROUND, MAX_TILE - done)
        out[t] = (done, nxt)
        summary = [summary[0] + nxt, summary[1] + (nxt > 0), summary[2] + rest]
    return out, tuple(summary)


def test_the_closed_loop(rt, torch_cuda, base):
    torch = torch_cuda
    stream = torch.cuda.current_stream().cuda_stream
    tiles = list(range(N_TILES))
    start = np.tile(np.array([0, FIRST], np.uint32), (N_TILES, 1))
    zero_cur = lambda img: img.cur.zero_()  # noqa: E731  ("old" of the first round: a cleared image)
    # ---- Level 2c, host-driven: one rt_trace_tile_work_delta per round, the statistics copied back, the rule on the host
    dev = rt.Device(0)
    try:
        dev.upload_scene(base["s"])
        himg, hdelta = Images(torch), poisoned_delta(torch)
        zero_cur(himg)
        counts, h_summaries, h_active = start.copy(), [], []
        for _ in range(ROUNDS):
            work = [(t, int(counts[t, 0]), min(int(counts[t, 1]), MAX_ROUND)) for t in tiles if counts[t, 1]]
            h_active.append({t for t, _, _ in work})
            if work:
                dev.trace_tile_work(base["cam"], work=work, width=W, height=H, max_bounce=B, delta_ptr=hdelta.data_ptr(),
                                    stream=stream, **himg.ptrs())
            torch.cuda.synchronize()
            counts, s = rule_numpy(counts, hdelta.cpu().numpy().view(np.uint32).reshape(-1, 4))
            h_summaries.append(s)
        hp, hc, hrays = himg.words()
        h_counts = counts
    finally:
        dev.close()
    # the condition that keeps the case meaningful: a tile at rest before round 4, a tile still traced in round 4
    print("active tiles per round", [len(a) for a in h_active], "summaries", h_summaries)
    assert len(h_active[3]) >= 1 and len(h_active[3]) < N_TILES
    assert any(t not in (0, 5, 10, 14, 15, 19) for t in set(tiles) - h_active[3])  # (not the dead tiles alone)
    assert 13 not in h_active[3] and {1, 7, 12} <= h_active[3]
    assert h_active[2] - h_active[3] or h_active[1] - h_active[2]
    assert h_summaries[-1][1] == 0 and h_summaries[-2][1] == 0  # (round 5 was the last that traced)
    # ---- Level 2d, device-driven: six rounds of trace + step enqueued with no host synchronisation
    dev = rt.Device(0)
    try:
        dev.upload_scene(base["s"])
        dimg, ddelta = Images(torch), poisoned_delta(torch)
        zero_cur(dimg)
        table = torch.from_numpy(start.view(np.int32).copy()).to("cuda")
        d_summary = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        h_slots = torch.full((ROUNDS, 4), -1, dtype=torch.int32).pin_memory()
        rule = rt.tile_rule(MAX_ROUND, MAX_TILE, REST_MAX_DELTA, U32)
        for r in range(ROUNDS):
            launch(dev, torch, base["cam"], tiles, table, MAX_ROUND, dimg, ddelta)
            rt.tile_counts_step(table.data_ptr(), ddelta.data_ptr(), W, H, rule, d_summary.data_ptr(), stream)
            h_slots[r].copy_(d_summary, non_blocking=True)  # 16 B, asynchronous: how a host learns when to stop
        info = dev.last_info()
        dp, dc, drays = dimg.words()
        d_counts = table.cpu().numpy().view(np.uint32)
        s = h_slots.numpy().view(rt.tile_step_summary_dtype).reshape(-1)
        d_summaries = [(int(x["NextFrames"]), int(x["ActiveTiles"]), int(x["RestedNow"])) for x in s]
    finally:
        dev.close()
    print("device summaries", d_summaries, "rays", drays, hrays)
    assert d_summaries == h_summaries
    assert np.array_equal(d_counts, h_counts) and (d_counts[:, 1] == 0).all()
    assert np.array_equal(dp, hp) and np.array_equal(dc, hc) and drays == hrays and drays > 0
    assert np.array_equal(ddelta.cpu().numpy(), hdelta.cpu().numpy())  # (each entry: its tile's last traced round)
    assert info["CullPassRan"] == 0 and info["TileCounts"] == 1, info  # (one key for the whole loop: one cull pass)


# ------------------------------------------------- 9. errors, with a device
def _raw_call(rt, dev, cam, img, tiles, table_ptr, max_frames, delta_ptr, *, n_tiles=None, band_count=1):
    c = rt.RtCameraInfo()
    ctypes.pointer(c)[0] = cam
    c.CurrentImage = rt.RtImage(img.cur.data_ptr(), img.w, img.h, rt.RT_FORMAT_R8G8B8A8_U32)
    c.PreviousImage = rt.RtImage(img.prev.data_ptr(), img.w, img.h, rt.RT_FORMAT_R32B32G32A32_F32)
    # (PreviousRayCount / Frames of the desc are not read: values rt_trace itself would refuse)
    d = rt.RtTraceDesc(img.w, img.h, 0xFFFFFFFF, 0xFFFFFFFF, B, 1, rt.RT_SEED_PIXEL, 32, band_count, 0, 0)
    arr = None if tiles is None else np.asarray(tiles, np.uint32)
    n = n_tiles if n_tiles is not None else (0 if arr is None else arr.size)
    vp = ctypes.c_void_p
    return rt.lib().rt_trace_tile_counts(dev.handle, ctypes.byref(c), ctypes.byref(d),
                                         vp(arr.ctypes.data if arr is not None and arr.size else None), n, vp(table_ptr),
                                         max_frames, vp(delta_ptr), vp(img.rays.data_ptr()),
                                         vp(img.torch.cuda.current_stream().cuda_stream))


def test_argument_errors_enqueue_nothing_and_leave_the_key(rt, torch_cuda, base):
    dev = rt.Device(0)
    try:
        dev.upload_scene(base["s"])
        table, delta = device_table(torch_cuda, TABLE_1), poisoned_delta(torch_cuda)
        img = Images(torch_cuda)
        launch(dev, torch_cuda, base["cam"], LIST_1, table, MAX_1, img, delta)
        assert dev.last_info()["CullPassRan"] == 1
        bad_img, bad_delta = Images(torch_cuda), poisoned_delta(torch_cuda)
        tp, dp = table.data_ptr(), bad_delta.data_ptr()
        for what, args, kw in (("NULL table", ([0, 7], None, 8, dp), {}), ("max_frames 0", ([0, 7], tp, 0, dp), {}),
                               ("misaligned d_delta", ([0, 7], tp, 8, dp + 4), {}),
                               ("a tile listed twice", ([3, 9, 3], tp, 8, dp), {}),
                               ("index 20", ([1, 20], tp, 8, dp), {}), ("BandCount 2", (LIST_1, tp, 8, dp), {"band_count": 2}),
                               ("NULL list", (None, tp, 8, dp), {"n_tiles": 2})):
            rc = _raw_call(rt, dev, base["cam"], bad_img, *args, **kw)
            assert rc == -22, (what, rc)
            assert rt.lib().rt_last_error(), what
            gp, gc, rays = bad_img.words()
            assert np.array_equal(gp, MEAN.view(np.uint32)) and np.all(gc == POISON) and rays == 0, what
            assert np.all(bad_delta.cpu().numpy().view(np.uint32) == POISON), what
            # the previous good call again: its key is still there
            img = Images(torch_cuda)
            launch(dev, torch_cuda, base["cam"], LIST_1, table, MAX_1, img, delta)
            assert_work(img, base["oracle"].expected(MIXED), what)
            assert dev.last_info()["CullPassRan"] == 0, what
        assert _raw_call(rt, dev, base["cam"], bad_img, None, tp, 8, dp) == 0  # n_tiles == 0
        assert _raw_call(rt, dev, base["cam"], bad_img, LIST_1, tp, 8, dp, n_tiles=0) == 0
        # no statistics (d_delta NULL), and the desc's own counts (values rt_trace refuses) are not read
        img = Images(torch_cuda)
        assert _raw_call(rt, dev, base["cam"], img, LIST_1, tp, MAX_1, None) == 0
        assert_work(img, base["oracle"].expected(MIXED), "raw call without statistics")
        assert dev.last_info()["CullPassRan"] == 0
    finally:
        dev.close()
