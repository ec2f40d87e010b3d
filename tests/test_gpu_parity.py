"""GPU parity: the HIP trace path vs the CPU oracle, through the C-ABI.

Bar (north star): output framebuffer within +-1 ULP per f32
channel, pixel addressing exact.  The kernel reproduces the oracle's f32
operation sequence exactly, so every test here asserts the stronger property:
BIT-EXACT accumulation (v4 f32), RGBA8 and bounce-segment counts.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gdev(rt, torch_cuda):
    dev = rt.Device(0)
    yield dev
    dev.close()


def _scenes(rt, orc, index, n=None):
    s = rt.scene_builtin(index)
    o = orc.scene_builtin(index)
    if n is not None:
        s = rt.scene_prefix(s, n)
        o = o.prefix(n)
    return s, o


def gpu_render(rt, torch, dev, scene, cam, W, H, *, frames, bounces, simd=True, prev_count=0, prev=None,
               band_rows=32, band_count=1, band_index=0, accum_zero=False, srgb_pow=False):
    dev.upload_scene(scene)
    local = rt.band_local_rows(H, band_rows, band_count, band_index)
    if prev is None:
        prev = torch.zeros((local * W, 4), dtype=torch.float32, device="cuda")
    cur = torch.zeros(local * W, dtype=torch.int32, device="cuda")
    rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    dev.trace(cam, width=W, height=H, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(), rays_ptr=rays.data_ptr(),
              prev_count=prev_count, frames=frames, max_bounce=bounces, simd=simd, band_rows=band_rows,
              band_count=band_count, band_index=band_index, accum_zero=accum_zero, srgb_pow=srgb_pow,
              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return prev, cur, int(rays.item())


def assert_same(gprev, gcur, grays, oprev, ocur, orays):
    gp = gprev.cpu().numpy().reshape(-1, 4)
    gc = gcur.cpu().numpy().view(np.uint32).reshape(-1)
    op = oprev.reshape(-1, 4)
    bad = np.argwhere(gp.view(np.uint32) != op.view(np.uint32))
    assert bad.size == 0, f"{len(bad)} accumulation words differ, first at {bad[:4].tolist()}: " \
                          f"gpu {gp[bad[0][0]]} oracle {op[bad[0][0]]}"
    assert np.array_equal(gc, ocur.reshape(-1)), f"{int((gc != ocur.reshape(-1)).sum())} RGBA8 pixels differ"
    assert grays == orays


CONFIGS = [
    # scene, N, W, H, spp, bounces, simd
    (1, 4, 256, 256, 1, 1, True),      # C1 geometry
    (1, 4, 256, 256, 1, 1, False),
    (1, 64, 128, 96, 8, 8, True),      # C2/C3 geometry, scaled image
    (1, 64, 128, 96, 8, 8, False),
    (1, 256, 64, 64, 2, 16, True),     # C5 geometry, scaled image (64 groups: per-group prefilter loop)
    (1, 100, 48, 40, 3, 8, False),     # 25 groups: clustered prefilter under the scalar rules
    (0, None, 96, 64, 4, 5, True),     # RGB Glass: dielectric + sticky inside flag
    (0, None, 96, 64, 4, 5, False),
    (2, None, 80, 48, 2, 5, True),     # RTWeekend: sky term, glass, 482 spheres
    (2, None, 80, 48, 2, 5, False),
    (1, 13, 37, 23, 3, 6, True),       # ragged N (padding lanes) and image not a tile multiple
    (1, 13, 37, 23, 3, 6, False),
    (1, 1, 1, 1, 4, 3, True),          # single pixel, single sphere
    # 32 / 50 groups: primary masks with bit 31 set (a sign-extended mask word once
    # tested groups past the scene: history-dependent misses at these sizes)
    (1, 128, 16, 16, 1, 1, True),
    (1, 128, 16, 8, 1, 1, True),
    (1, 200, 40, 32, 3, 8, True),
    (1, 200, 40, 32, 3, 8, False),
]


@pytest.mark.parametrize("scene_idx,n,W,H,spp,B,simd", CONFIGS)
def test_parity_vs_oracle(rt, orc, torch_cuda, gdev, scene_idx, n, W, H, spp, B, simd):
    s, o = _scenes(rt, orc, scene_idx, n)
    cam = rt.camera_setup(s, W, H)
    g = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=spp, bounces=B, simd=simd)
    r = orc.render(o, orc.camera(o, W, H), W, H, frames=spp, max_bounce=B, simd=simd)
    assert_same(*g, *r)


def test_progressive_split_equals_single_launch(rt, orc, torch_cuda, gdev):
    """Frames 0-2 then 3-7 (PreviousRayCount=3, accumulation read back from HBM)
    equal one 8-frame launch and the oracle: the running-mean fold order is kept."""
    s, o = _scenes(rt, orc, 1, 64)
    W, H = 64, 48
    cam = rt.camera_setup(s, W, H)
    p1, c1, r1 = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=3, bounces=8)
    p2, c2, r2 = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=5, bounces=8, prev_count=3, prev=p1)
    pa, ca, ra = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=8, bounces=8)
    assert torch_cuda.equal(p2, pa) and torch_cuda.equal(c2, ca) and r1 + r2 == ra
    r = orc.render(o, orc.camera(o, W, H), W, H, frames=8, max_bounce=8)
    assert_same(pa, ca, ra, *r)


@pytest.mark.parametrize("scene_idx,n,W,H,G", [(0, None, 203, 77, 1), (1, 64, 150, 70, 1), (2, None, 96, 88, 3),
                                                (1, 64, 200, 150, 8)])
def test_one_frame_launches_take_four_pixels_per_lane(rt, orc, torch_cuda, gdev, scene_idx, n, W, H, G):
    """The OnRender unit: launches of ONE frame (PreviousRayCount 0, 1, 2, as
    OnRender folds them) run one lane per pixel with 4 pixels per lane over
    16x16 wave tiles (rt_trace_info.PixelsPerLane); ragged images leave some
    lanes' later pixel slots outside the image, and 8-row bands of G devices
    make a wave tile span two bands (its cull cone covers both).  The running
    mean and RGBA8 of every frame equal the oracle's, bit for bit."""
    torch = torch_cuda
    s, o = _scenes(rt, orc, scene_idx, n)
    cam = rt.camera_setup(s, W, H)
    ocam = orc.camera(o, W, H)
    band_rows = 8 if G > 1 else 32
    for r in range(G):
        local = rt.band_local_rows(H, band_rows, G, r)
        prev = torch.zeros((local * W, 4), dtype=torch.float32, device="cuda")
        rows = [y for y in range(H) if (y // band_rows) % G == r]
        for k in range(3):
            g = gpu_render(rt, torch, gdev, s, cam, W, H, frames=1, bounces=5, prev_count=k, prev=prev,
                           band_rows=band_rows, band_count=G, band_index=r)
            assert gdev.last_info()["PixelsPerLane"] == 4
            op, oc, _ = orc.render(o, ocam, W, H, frames=k + 1, max_bounce=5)
            op = op.reshape(H, W, 4)[rows].reshape(-1, 4)
            oc = oc.reshape(H, W)[rows].reshape(-1)
            gp = g[0].cpu().numpy().reshape(-1, 4)
            assert np.array_equal(gp.view(np.uint32), op.view(np.uint32)), (r, k)
            assert np.array_equal(g[1].cpu().numpy().view(np.uint32), oc), (r, k)


@pytest.mark.parametrize("order,xcd,seg", [(1, 1, 1), (1, -1, 1), (-1, 1, 1), (1, 1, 2), (1, 1, 4)])
@pytest.mark.parametrize("scene_idx,n,W,H,spp,B,lpp", [(1, 64, 96, 80, 8, 8, 4), (2, None, 72, 56, 8, 5, 4),
                                                       (0, None, 64, 48, 16, 5, 8), (1, 200, 40, 32, 16, 8, 16)])
def test_pixels_dealt_by_cost_keep_every_bit(rt, orc, torch_cuda, scene_idx, n, W, H, spp, B, lpp, order, xcd, seg):
    """PixelSort on: after a launch measures each pixel's traced segments,
    every block tile's pixels are dealt to its four waves cheapest first (and
    a permuted wave tests the union of the block's quadrant masks).  Repeated
    launches with the permutation in place equal the oracle bit for bit."""
    dev = rt.Device(0, options={"PixelSort": rt.RT_OPT_ON, "LanesPerPixel": lpp,
                                "WaveOrder": order,  # waves ordered by cost, or block tiles
                                "XcdGroup": xcd,  # a block tile's waves grouped onto one XCD (wave order only)
                                "PixelSegment": seg})  # pixels dealt singly, in pairs or in 4-pixel row segments
    try:
        s, o = _scenes(rt, orc, scene_idx, n)
        cam = rt.camera_setup(s, W, H)
        r = orc.render(o, orc.camera(o, W, H), W, H, frames=spp, max_bounce=B)
        dev.upload_scene(s)
        torch = torch_cuda
        sorted_launches = 0
        for _ in range(4):
            prev = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
            cur = torch.zeros(W * H, dtype=torch.int32, device="cuda")
            rays = torch.zeros(1, dtype=torch.int64, device="cuda")
            dev.trace(cam, width=W, height=H, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(),
                      rays_ptr=rays.data_ptr(), frames=spp, max_bounce=B, accum_zero=True,
                      stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert_same(prev, cur, int(rays.item()), *r)
            sorted_launches += dev.last_info()["PixelsSorted"]
        assert sorted_launches == 3
    finally:
        dev.close()


def test_accum_zero_flag_ignores_stale_buffer(rt, orc, torch_cuda, gdev):
    s, o = _scenes(rt, orc, 1, 16)
    W, H = 32, 32
    cam = rt.camera_setup(s, W, H)
    junk = torch_cuda.full((W * H, 4), float("nan"), device="cuda")
    g = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=2, bounces=4, prev=junk, accum_zero=True)
    r = orc.render(o, orc.camera(o, W, H), W, H, frames=2, max_bounce=4)
    assert_same(*g, *r)


@pytest.mark.parametrize("G", [2, 3, 8])
def test_band_partition_and_assembly(rt, orc, torch_cuda, gdev, G):
    """Per-GPU interleaved 32-row bands traced separately and
    assembled equal the single-device image bit for bit."""
    torch = torch_cuda
    s, o = _scenes(rt, orc, 1, 64)
    W, H = 72, 150  # 5 bands, the last one partial
    cam = rt.camera_setup(s, W, H)
    rows = [rt.band_local_rows(H, 32, G, r) for r in range(G)]
    assert sum(rows) == H
    maxr = max(rows)
    stride4, stride16 = maxr * W * 4, maxr * W * 16
    cur_all = torch.zeros(G * maxr * W, dtype=torch.int32, device="cuda")
    prev_all = torch.zeros((G * maxr * W, 4), dtype=torch.float32, device="cuda")
    total = 0
    for r in range(G):
        if rows[r] == 0:
            continue
        p, c, n = gpu_render(rt, torch, gdev, s, cam, W, H, frames=2, bounces=8, band_count=G, band_index=r)
        cur_all[r * maxr * W: r * maxr * W + rows[r] * W] = c
        prev_all[r * maxr * W: r * maxr * W + rows[r] * W] = p
        total += n
    cur = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    prev = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rt.assemble_bands(cur_all.data_ptr(), stride4, cur.data_ptr(), W, H, 4, 32, G, stream=st)
    rt.assemble_bands(prev_all.data_ptr(), stride16, prev.data_ptr(), W, H, 16, 32, G, stream=st)
    torch.cuda.synchronize()
    r = orc.render(o, orc.camera(o, W, H), W, H, frames=2, max_bounce=8)
    assert_same(prev, cur, total, *r)


def test_zero_bounces_and_zero_frames(rt, orc, torch_cuda, gdev):
    s, o = _scenes(rt, orc, 1, 8)
    W, H = 16, 8
    cam = rt.camera_setup(s, W, H)
    g = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=3, bounces=0)
    r = orc.render(o, orc.camera(o, W, H), W, H, frames=3, max_bounce=0)
    assert_same(*g, *r)
    p, c, n = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=0, bounces=5)
    assert n == 0 and int(c.abs().sum()) == 0


def test_full_hd_rows_match_oracle(rt, orc, torch_cuda, gdev):
    """C2 at full size (1920x1080, 64 spheres, 8 bounces) for 16 spp: rows
    sampled across the frame match the oracle, which renders only those rows."""
    s, o = _scenes(rt, orc, 1, 64)
    W, H, S, B = 1920, 1080, 16, 8
    cam = rt.camera_setup(s, W, H)
    gp, gc, _ = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=S, bounces=B)
    gp = gp.cpu().numpy().reshape(H, W, 4)
    gc = gc.cpu().numpy().view(np.uint32).reshape(H, W)
    ocam = orc.camera(o, W, H)
    for y0 in (0, 517, 1078):
        op, oc, _ = orc.render(o, ocam, W, H, frames=S, max_bounce=B, rows=(y0, y0 + 2), threads=orc.cpu_threads())
        op = op.reshape(H, W, 4)[y0:y0 + 2]
        oc = oc.reshape(H, W)[y0:y0 + 2]
        assert np.array_equal(gp[y0:y0 + 2].view(np.uint32), op.view(np.uint32)), y0
        assert np.array_equal(gc[y0:y0 + 2], oc), y0


def test_c5_rows_match_oracle(rt, orc, torch_cuda, gdev):
    """C5's geometry at full size (7680x4320, 256 spheres, 16 bounces; 4 of its
    4096 spp -- later frames run the same code with other seeds): rows across
    the frame match the oracle, which renders only those rows."""
    s, o = _scenes(rt, orc, 1, 256)
    W, H, S, B = 7680, 4320, 4, 16
    cam = rt.camera_setup(s, W, H)
    gp, gc, _ = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=S, bounces=B)
    gp = gp.cpu().numpy().reshape(H, W, 4)
    gc = gc.cpu().numpy().view(np.uint32).reshape(H, W)
    ocam = orc.camera(o, W, H)
    for y0 in (0, 2161, 4318):
        op, oc, _ = orc.render(o, ocam, W, H, frames=S, max_bounce=B, rows=(y0, y0 + 2), threads=orc.cpu_threads())
        op = op.reshape(H, W, 4)[y0:y0 + 2]
        oc = oc.reshape(H, W)[y0:y0 + 2]
        assert np.array_equal(gp[y0:y0 + 2].view(np.uint32), op.view(np.uint32)), y0
        assert np.array_equal(gc[y0:y0 + 2], oc), y0


def test_on_render_progressive_driver(rt, orc, torch_cuda):
    """OnRender semantics (main.cpp:705-859): first call resets and renders
    frame 0 without output; each later call returns the previous COMPLETED
    frame; a scene switch resets the running mean."""
    rt.on_init()
    W, H = 48, 40
    img = np.zeros((H, W), np.uint32)
    o = orc.scene_builtin(1)
    ocam = orc.camera(o, W, H)
    done, _, _ = rt.on_render(img, 1)
    assert not done
    frames = []
    for k in range(3):
        rt.on_render_wait()
        done, rays, _ = rt.on_render(img, 1)
        assert done
        frames.append((img.copy(), rays))
    for k, (im, rays) in enumerate(frames):
        _, ocur, orays = orc.render(o, ocam, W, H, frames=k + 1, max_bounce=5)
        assert np.array_equal(im.reshape(-1), ocur), k
    # scene switch -> reset: the next completed frame is frame 0 of scene 0
    rt.on_render_wait()
    rt.on_render(img, 0)
    rt.on_render_wait()
    done, _, _ = rt.on_render(img, 0)
    assert done
    o0 = orc.scene_builtin(0)
    _, ocur0, _ = orc.render(o0, orc.camera(o0, W, H), W, H, frames=1, max_bounce=5)
    assert np.array_equal(img.reshape(-1), ocur0)
    rt.on_render_wait()
    rt.on_shutdown()


def test_on_render_busy_poll_hands_out_every_frame_in_order(rt, orc, torch_cuda):
    """The platform loop without waits (bench.py --config onrender): calls that
    find the frame still tracing return 0; every completed frame handed out is
    the progressive mean over one more frame, while the next one already traces
    in the other device slot."""
    rt.on_init()
    try:
        W, H = 64, 48
        img = np.zeros((H, W), np.uint32)
        o = orc.scene_builtin(1)
        ocam = orc.camera(o, W, H)
        rt.on_render(img, 1)
        got = []
        for _ in range(200000):
            done, rays, _ = rt.on_render(img, 1)
            if done:
                got.append((img.copy(), rays))
                if len(got) == 4:
                    break
        assert len(got) == 4
        for k, (im, rays) in enumerate(got):
            _, ocur, orays = orc.render(o, ocam, W, H, frames=k + 1, max_bounce=5)
            assert np.array_equal(im.reshape(-1), ocur), k
        rt.on_render_wait()
    finally:
        rt.on_shutdown()


def test_on_render_fresh_image_every_call_and_registered_image(rt, orc, torch_cuda):
    """A new host array on every call (freed buffers can come back at the same
    address) gets every frame through the library's staging buffer: the
    library page-locks nothing it was not handed.  A registered image gets the
    same frames by DMA; after unregistering, the staged path serves it again."""
    rt.on_init()
    try:
        W, H = 64, 40
        o = orc.scene_builtin(0)
        ocam = orc.camera(o, W, H)
        rt.on_render(np.zeros((H, W), np.uint32), 0)
        want = [orc.render(o, ocam, W, H, frames=k + 1, max_bounce=5)[1] for k in range(6)]
        for k in range(6):
            if k == 2:
                reg = np.zeros((H, W), np.uint32)
                rt.on_render_register_image(reg)
            if k == 4:
                rt.on_render_unregister_image()
            img = reg if k in (2, 3) else np.full((H, W), 0xDEADBEEF, np.uint32)
            rt.on_render_wait()
            done, _, _ = rt.on_render(img, 0)
            assert done
            assert np.array_equal(img.reshape(-1), want[k]), k
            del img
        rt.on_render_wait()
    finally:
        rt.on_shutdown()


def test_on_render_moving_camera_restarts_every_frame(rt, orc, torch_cuda):
    """RT_KEY_LEFT on every call (main.cpp:743-746): each call turns the camera
    by 1/16 rad, restarts the mean, and hands out the previous call's frame --
    one frame under the previous call's camera."""
    rt.on_init()
    try:
        W, H = 56, 40
        img = np.zeros((H, W), np.uint32)
        o = orc.scene_builtin(2)
        angle = np.float32(o.x_angle)
        angles = []
        for j in range(4):
            angle = np.float32(angle + np.float32(1.0 / 16.0))  # the key's f32 step
            angles.append(angle)
            done, _, _ = rt.on_render(img, 2, keys=rt.KEY_LEFT)
            assert done == (j > 0)
            if j > 0:
                ocam = orc.camera(o, W, H, x_angle=float(angles[j - 1]))
                _, ocur, _ = orc.render(o, ocam, W, H, frames=1, max_bounce=5)
                assert np.array_equal(img.reshape(-1), ocur), j
        rt.on_render_wait()
    finally:
        rt.on_shutdown()


# Kernel variants selected at device creation through the C-ABI (rt_device_options,
# rt_device_create_ex; 1 = RT_OPT_ON, -1 = RT_OPT_OFF): prefilter forced on/off,
# brute-force primaries, 1/2/16/32 lanes per pixel, the LDS-staged sphere source,
# four-wave workgroups, the run-time walk dispatch.  Every variant must give the
# same bits as the oracle.
ON, OFF = 1, -1
VARIANT_OPTIONS = [{"Prefilter": ON}, {"Prefilter": OFF}, {"Clusters": OFF}, {"Clusters": ON},
                   {"Interleave": ON}, {"Cull": OFF}, {"LanesPerPixel": 1}, {"LanesPerPixel": 2},
                   {"LanesPerPixel": 32}, {"SecondaryThreshold": 1}, {"SphereSourceLds": ON},
                   {"SphereSourceLds": ON, "Cull": OFF}, {"SphereSourceLds": ON, "Clusters": OFF},
                   {"SceneInHbm": ON}, {"SceneInHbm": ON, "Cull": OFF},
                   # four-wave workgroups with the LDS image (the default is one wave per
                   # workgroup, each kernel compiled for one secondary walk)
                   {"OneWaveGroups": OFF}, {"OneWaveGroups": OFF, "Clusters": ON}, {"WalkAny": ON},
                   {"WalkAny": ON, "Clusters": ON}, {"LanesPerPixel": 16, "Clusters": ON},
                   # 4 pixels per lane at every frame count (the one-frame launch shape), and never
                   {"LanesPerPixel": 1, "PixelsPerLane": 4}, {"PixelsPerLane": 1},
                   # merged primary/secondary rounds forced on (every per-group-walk kernel) and off
                   {"MergeRounds": ON, "Clusters": OFF}, {"MergeRounds": OFF}, {"PixelSort": OFF},
                   # block tiles ordered by cost instead of waves
                   {"WaveOrder": OFF},
                   # round 5: RGBA8 stored by the trace kernel (no encode pass); pixel pairs / 4-pixel
                   # row segments dealt by cost; waves not grouped by XCD
                   {"EncodePass": OFF}, {"PixelSegment": 2}, {"PixelSegment": 4}, {"XcdGroup": OFF},
                   # round 6: the brute-force roofline's kernel (bench.py --brute), the XCD grouping
                   # without the cull pass (its live-tile total written by the host), the cluster
                   # table's K and sub-cluster size
                   {"Cull": OFF, "Prefilter": OFF}, {"Cull": OFF, "XcdGroup": ON},
                   {"ClusterCount": 3, "SubClusterSpheres": 2}]


@pytest.mark.parametrize("options", VARIANT_OPTIONS, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_kernel_variants_match_oracle(rt, orc, torch_cuda, options):
    dev = rt.Device(0, options=options)
    assert dev.options() == options
    try:
        # (1, 200): 50 groups, the two-word cluster mask with Clusters on
        for scene_idx, n, W, H, spp, B in [(1, 64, 64, 48, 6, 8), (1, 200, 40, 32, 3, 8), (0, None, 48, 32, 4, 5),
                                           (2, None, 40, 24, 2, 5)]:
            for simd in (True, False):
                s, o = _scenes(rt, orc, scene_idx, n)
                cam = rt.camera_setup(s, W, H)
                g = gpu_render(rt, torch_cuda, dev, s, cam, W, H, frames=spp, bounces=B, simd=simd)
                r = orc.render(o, orc.camera(o, W, H), W, H, frames=spp, max_bounce=B, simd=simd)
                assert_same(*g, *r)
    finally:
        dev.close()


def test_tiny_sphere_scene_takes_the_ieee_sqrt(rt, orc, torch_cuda, gdev):
    """A sphere with r^2 below 2^-36 puts candidate square roots outside the
    short sequence's verified range: the host must fall back (flag bit 1
    clear) and the result stays exact."""
    base = rt.scene_prefix(rt.scene_builtin(1), 16)
    sp, _, _ = rt.scene_arrays(base)
    sp = sp.copy()
    sp[3, 4] = np.float32(2e-6)  # radius -> r^2 = 4e-12 < 2^-36
    s = rt.scene_from_spheres(sp, look_at=(base.LookAt.x, base.LookAt.y, base.LookAt.z),
                              distance=base.DefaultDistanceFromLookAt, x_angle=base.DefaultXAngle,
                              y_height=base.DefaultYHeight)
    for simd in (True, False):
        assert not (rt.scene_prefilter(s, simd)[2] & 2)
    _, groups, mats = rt.scene_arrays(s)
    o = orc.Scene(sp, groups, mats, look_at=(base.LookAt.x, base.LookAt.y, base.LookAt.z),
                  distance=base.DefaultDistanceFromLookAt, x_angle=base.DefaultXAngle,
                  y_height=base.DefaultYHeight)
    W, H = 64, 48
    cam = rt.camera_setup(s, W, H)
    for simd in (True, False):
        g = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=4, bounces=8, simd=simd)
        r = orc.render(o, orc.camera(o, W, H), W, H, frames=4, max_bounce=8, simd=simd)
        assert_same(*g, *r)


@pytest.mark.parametrize("scene_idx,n", [(1, 64), (1, 256), (0, None)])
def test_cone_culling_is_exact_at_full_resolution(rt, orc, torch_cuda, scene_idx, n):
    """Primary-ray cone culling (tight f64 cones, per 4x4 / 2x2 tile) and the
    empty-tile fast path must not change a single bit at the BASELINE
    resolution: the culled kernel against the brute-force one (Cull off),
    full 1920x1080 frame, several lanes-per-pixel shapes."""
    s, _ = _scenes(rt, orc, scene_idx, n)
    W, H = 1920, 1080
    cam = rt.camera_setup(s, W, H)
    out = {}
    for opts in ({"Cull": OFF, "LanesPerPixel": 4}, {"LanesPerPixel": 4}, {"LanesPerPixel": 16},
                 {"LanesPerPixel": 1}):
        dev = rt.Device(0, options=opts)
        try:
            out[tuple(opts.items())] = gpu_render(rt, torch_cuda, dev, s, cam, W, H, frames=3, bounces=8)
        finally:
            dev.close()
    ref = out[(("Cull", OFF), ("LanesPerPixel", 4))]
    for key, g in out.items():
        assert torch_cuda.equal(g[0], ref[0]) and torch_cuda.equal(g[1], ref[1]) and g[2] == ref[2], key


@pytest.mark.parametrize("lpp", [4, 16, 32])
def test_tile_order_from_previous_launch_keeps_every_bit(rt, orc, torch_cuda, lpp):
    """Repeated launches of one geometry run their tiles heaviest-first (order
    learned from the previous launch): the image, the accumulation and the ray
    count must equal the identity-order launch bit for bit, launch after launch."""
    s, _ = _scenes(rt, orc, 1, 64)
    W, H = 640, 360
    cam = rt.camera_setup(s, W, H)
    dev0 = rt.Device(0, options={"LanesPerPixel": lpp, "TileOrder": OFF})
    try:
        ref = gpu_render(rt, torch_cuda, dev0, s, cam, W, H, frames=6, bounces=8)
    finally:
        dev0.close()
    dev = rt.Device(0, options={"LanesPerPixel": lpp, "TileOrder": ON})
    try:
        for _ in range(4):
            g = gpu_render(rt, torch_cuda, dev, s, cam, W, H, frames=6, bounces=8)
            assert torch_cuda.equal(g[0], ref[0]) and torch_cuda.equal(g[1], ref[1]) and g[2] == ref[2]
    finally:
        dev.close()


def test_dead_tiles_fold_a_nonzero_running_mean(rt, orc, torch_cuda, gdev):
    """Pixels of tiles no primary ray can hit go through rtk_launch_empty; with a
    random non-zero accumulation (PreviousRayCount 5) they must blend zeros
    exactly like the oracle's traced misses."""
    s, o = _scenes(rt, orc, 1, 64)
    W, H = 256, 192
    cam = rt.camera_setup(s, W, H)
    rng = np.random.default_rng(11)
    prev_np = rng.uniform(0.0, 2.0, (W * H, 4)).astype(np.float32)
    prev = torch_cuda.from_numpy(prev_np.copy()).to("cuda")
    g = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=3, bounces=4, prev_count=5, prev=prev)
    r = orc.render(o, orc.camera(o, W, H), W, H, prev_count=5, frames=3, max_bounce=4, prev=prev_np.copy())
    assert_same(*g, *r)


@pytest.mark.parametrize("prev_count,P", [(65533, 4), (65530, 16), (1000003, 4), (16777217, 16), (300000001, 1),
                                          (4294967000, 8)])
def test_running_mean_weights_at_large_previous_counts(rt, orc, torch_cuda, prev_count, P):
    """The fold weights RN(1/(f32)(n)) and RN((f32)(n-1)/(f32)(n)) (main.cpp:484-487)
    come from the device's static table of the first 65,536 frames (TraceArgs.weights)
    and past it from rcp_rn / div_rn (rtk_math.h fold_weights) in the one-wave
    kernels: launches across the table's end, frames far past it, counts whose f32
    conversion rounds (> 2^24) and the top of the u32 range, against the oracle's IEEE
    divisions, with a random non-zero running mean, every lane shape's blend path."""
    s, o = _scenes(rt, orc, 1, 64)
    W, H = 64, 48
    cam = rt.camera_setup(s, W, H)
    rng = np.random.default_rng(prev_count % 1000)
    prev_np = rng.uniform(0.0, 2.0, (W * H, 4)).astype(np.float32)
    prev = torch_cuda.from_numpy(prev_np.copy()).to("cuda")
    dev = rt.Device(0, options={"LanesPerPixel": P})
    try:
        g = gpu_render(rt, torch_cuda, dev, s, cam, W, H, frames=P, bounces=4, prev_count=prev_count, prev=prev)
    finally:
        dev.close()
    r = orc.render(o, orc.camera(o, W, H), W, H, prev_count=prev_count, frames=P, max_bounce=4, prev=prev_np.copy())
    assert_same(*g, *r)


def test_camera_change_recomputes_the_cull_pass(rt, orc, torch_cuda, gdev):
    """The cull masks and live-tile list are cached per camera / scene /
    geometry: moving the camera between launches on one device must re-cull."""
    s, o = _scenes(rt, orc, 1, 64)
    W, H = 128, 96
    for dist, ang in [(None, None), (6.0, 0.7), (None, None)]:
        cam = rt.camera_setup(s, W, H, distance=dist, x_angle=ang)
        g = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=2, bounces=5)
        r = orc.render(o, orc.camera(o, W, H, distance=dist, x_angle=ang), W, H, frames=2, max_bounce=5)
        assert_same(*g, *r)


@pytest.mark.parametrize("simd", [True, False])
def test_new_cameras_back_to_back_without_host_sync(rt, orc, torch_cuda, simd):
    """Three different cameras enqueued back to back with no synchronisation in
    between: each is a new cull key whose live-tile count stays
    on the device (grid over every tile, early exit), and its dead-tile segments
    are added from the device total.  The long launches also take the split
    head + rest path.  Every frame and count is bit-exact vs the oracle; the
    folded segments reported afterwards (rt_trace_last_info, which waits for the
    totals) are the last camera's."""
    torch = torch_cuda
    s, o = _scenes(rt, orc, 1, 64)
    W, H, F, B = 160, 96, 128, 5
    views = [(None, None), (6.0, 0.7), (2.0, -1.1)]
    dev = rt.Device(0, options={"LanesPerPixel": 4})  # P = 4: a 128-frame launch is split (head + rest)
    try:
        dev.upload_scene(s)
        stream = torch.cuda.current_stream().cuda_stream
        outs = []
        for dist, ang in views:
            cam = rt.camera_setup(s, W, H, distance=dist, x_angle=ang)
            prev = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
            cur = torch.zeros(W * H, dtype=torch.int32, device="cuda")
            rays = torch.zeros(1, dtype=torch.int64, device="cuda")
            dev.trace(cam, width=W, height=H, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(),
                      rays_ptr=rays.data_ptr(), frames=F, max_bounce=B, simd=simd, accum_zero=True, stream=stream)
            outs.append((prev, cur, rays))
        info = dev.last_info()
        torch.cuda.synchronize()
    finally:
        dev.close()
    assert info["CullPassRan"] == 1 and info["SplitHeadFrames"] > 0, info
    for (dist, ang), (prev, cur, rays) in zip(views, outs):
        r = orc.render(o, orc.camera(o, W, H, distance=dist, x_angle=ang), W, H, frames=F, max_bounce=B, simd=simd)
        assert_same(prev, cur, int(rays.item()), *r)
    assert 0 < info["TilesTraced"] <= info["TilesTotal"]


def test_stream_switch_keeps_every_bit(rt, orc, torch_cuda):
    """Launches of one device on two streams in turn: the new stream waits for
    the old one's last trace on the device (no host synchronisation, the cull
    masks and learned order are kept)."""
    torch = torch_cuda
    s, o = _scenes(rt, orc, 1, 64)
    W, H = 96, 64
    cam = rt.camera_setup(s, W, H)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    dev = rt.Device(0)
    try:
        dev.upload_scene(s)
        outs = []
        for i in range(4):
            prev = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
            cur = torch.zeros(W * H, dtype=torch.int32, device="cuda")
            rays = torch.zeros(1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            dev.trace(cam, width=W, height=H, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(),
                      rays_ptr=rays.data_ptr(), frames=4, max_bounce=5, accum_zero=True,
                      stream=streams[i % 2].cuda_stream)
            outs.append((prev, cur, rays))
        torch.cuda.synchronize()
    finally:
        dev.close()
    r = orc.render(o, orc.camera(o, W, H), W, H, frames=4, max_bounce=5)
    for prev, cur, rays in outs:
        assert_same(prev, cur, int(rays.item()), *r)


@pytest.mark.parametrize("idx,n,W,H,P", [(1, 64, 96, 64, 4), (1, 128, 16, 16, 1), (1, 200, 40, 32, 2),
                                         (1, 256, 64, 48, 8), (0, None, 48, 32, 16)])
def test_cull_masks_equal_cpu_restatement(rt, torch_cuda, idx, n, W, H, P):
    """The cull pass's primary sphere-pair masks (rt_debug_masks) equal the numpy
    f64 restatement (tests/cull_ref.py) word for word; tests/test_cull_bound.py
    checks that restatement keeps every pair a pixel's rays can reach."""
    from cull_ref import np_masks
    s = rt.scene_builtin(idx)
    if n:
        s = rt.scene_prefix(s, n)
    cam = rt.camera_setup(s, W, H)
    dev = rt.Device(0, options={"LanesPerPixel": P})
    try:
        gpu_render(rt, torch_cuda, dev, s, cam, W, H, frames=1, bounces=1)
        got = dev.debug_masks()
    finally:
        dev.close()
    ref = np_masks(rt, s, cam, W, H, P)
    assert got is not None and np.array_equal(got, ref), np.flatnonzero(got != ref)[:8]


@pytest.mark.parametrize("simd", [True, False])
def test_srgb_pow_flag_changes_only_the_rgba8(rt, orc, torch_cuda, gdev, simd):
    """RT_FLAG_SRGB_POW (main.cpp:320-321): the running mean and ray count are
    those of the default path; the RGBA8 is the oracle's pow-branch encoding."""
    s, o = _scenes(rt, orc, 0)
    W, H = 64, 48
    cam = rt.camera_setup(s, W, H)
    gp, gc, gr = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=3, bounces=5, simd=simd, srgb_pow=True)
    op, oc, orays = orc.render(o, orc.camera(o, W, H), W, H, frames=3, max_bounce=5, simd=simd)
    ocp = orc.encode_rgba8(op, srgb_pow=True)
    assert not np.array_equal(ocp, oc.reshape(-1))
    assert_same(gp, gc, gr, op, ocp, orays)


def test_encode_rgba8_exhaustive(rt, orc, torch_cuda):
    """rt_encode_rgba8 over every f32 the pow branch sees ([0.0031308, 1], three
    per pixel) plus edge values, both curves: bytes equal the oracle's."""
    torch = torch_cuda
    lo = np.array([0.0031308], np.float32).view(np.uint32)[0]
    vals = np.arange(lo, 0x3F800000 + 1, dtype=np.uint32).view(np.float32)
    edge = np.array([-1.0, -0.0, 0.0, 1e-30, 0.001, 2.0, np.inf, -np.inf, np.nan], np.float32)
    vals = np.concatenate([vals, edge, np.zeros((-(len(vals) + len(edge))) % 3, np.float32)])
    v4 = np.ones((len(vals) // 3, 4), np.float32)
    v4[:, :3] = vals.reshape(-1, 3)
    d_in = torch.from_numpy(v4).cuda()
    d_out = torch.zeros(len(v4), dtype=torch.int32, device="cuda")
    for pw in (True, False):
        rt.encode_rgba8(d_in.data_ptr(), d_out.data_ptr(), len(v4), srgb_pow=pw,
                        stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(np.uint32)
        want = orc.encode_rgba8(v4, srgb_pow=pw)
        assert np.array_equal(got, want), f"pow={pw}: {int((got != want).sum())} pixels differ"


@pytest.mark.parametrize("n_groups", [164, 265])
def test_largest_scene_the_lds_image_holds(rt, orc, torch_cuda, n_groups):
    """164 groups (656 spheres) is the LDS-staged maximum of the four-wave
    kernels (rt_kernel.h kMaxLdsGroups, 64-B sphere records); 265 groups stay
    in HBM.  RTWeekend's 482 spheres plus (or, at 164 groups, minus) small
    spheres scattered over its ground (materials copied from RTWeekend's),
    both rule sets, traced by the four-wave kernels that stage the image."""
    gdev = rt.Device(0, options={"OneWaveGroups": OFF})
    base = rt.scene_builtin(2)
    sp0, _, _ = rt.scene_arrays(base)
    rng = np.random.default_rng(265)
    n = 4 * n_groups
    extra = sp0[rng.integers(1, len(sp0), max(n - len(sp0), 0))].copy()
    extra[:, 0] = rng.uniform(-1.5, 1.5, len(extra))  # the scene is at 1/16 scale
    extra[:, 2] = rng.uniform(-1.5, 1.5, len(extra))
    extra[:, 4] = rng.uniform(0.005, 0.02, len(extra))
    extra[:, 1] = extra[:, 4]
    sp = np.concatenate([sp0, extra]).astype(np.float32)[:n]
    la = (base.LookAt.x, base.LookAt.y, base.LookAt.z)
    kw = dict(distance=base.DefaultDistanceFromLookAt, x_angle=base.DefaultXAngle, y_height=base.DefaultYHeight)
    s = rt.scene_from_spheres(sp, look_at=la, use_sky=True, **kw)
    _, groups, mats = rt.scene_arrays(s)
    assert len(groups) == n_groups
    o = orc.Scene(sp, groups, mats, look_at=la, use_sky=True, **kw)
    W, H = 48, 32
    cam = rt.camera_setup(s, W, H)
    try:
        for simd in (True, False):
            g = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=2, bounces=5, simd=simd)
            r = orc.render(o, orc.camera(o, W, H), W, H, frames=2, max_bounce=5, simd=simd)
            assert_same(*g, *r)
    finally:
        gdev.close()


def test_upload_waits_for_traces_in_flight(rt, orc, torch_cuda):
    """rt_trace is asynchronous on the caller's stream; rt_scene_upload writes
    through the device's own stream.  Uploading scene B right after enqueueing
    a trace of scene A (no synchronisation in between, same allocation size)
    must not change A's frame: both frames equal the oracle's."""
    torch = torch_cuda
    sa, oa = _scenes(rt, orc, 1, 64)
    spb, _, _ = rt.scene_arrays(sa)
    spb = spb.copy()
    spb[:, 1] += np.float32(0.05)  # same sphere count, every centre moved
    sb = rt.scene_from_spheres(spb, look_at=(sa.LookAt.x, sa.LookAt.y, sa.LookAt.z),
                               distance=sa.DefaultDistanceFromLookAt, x_angle=sa.DefaultXAngle,
                               y_height=sa.DefaultYHeight)
    _, gb, mb = rt.scene_arrays(sb)
    ob = orc.Scene(spb, gb, mb, look_at=(sa.LookAt.x, sa.LookAt.y, sa.LookAt.z), distance=sa.DefaultDistanceFromLookAt,
                   x_angle=sa.DefaultXAngle, y_height=sa.DefaultYHeight)
    W, H, S, B = 320, 240, 16, 8
    cam = rt.camera_setup(sa, W, H)
    dev = rt.Device(0)
    side = torch.cuda.Stream()
    try:
        out = []
        dev.upload_scene(sa)
        for scene in (sb, None):
            prev = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
            cur = torch.zeros(W * H, dtype=torch.int32, device="cuda")
            rays = torch.zeros(1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                dev.trace(cam, width=W, height=H, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(),
                          rays_ptr=rays.data_ptr(), frames=S, max_bounce=B, stream=side.cuda_stream)
            if scene is not None:
                dev.upload_scene(scene)  # no synchronisation with `side` by the caller
            side.synchronize()
            out.append((prev, cur, int(rays.item())))
    finally:
        dev.close()
    for (p, c, n), o in zip(out, (oa, ob)):
        r = orc.render(o, orc.camera(o, W, H), W, H, frames=S, max_bounce=B)
        assert_same(p, c, n, *r)


@pytest.mark.parametrize("n_spheres", [1061, 2000, 4099, 9001])
def test_scene_beyond_the_lds_image(rt, orc, torch_cuda, gdev, n_spheres):
    """Scenes above 656 spheres (164 groups) stay in HBM even for the four-wave
    kernels (the one-wave default keeps every scene there): the sphere loop
    reads groups through the scalar cache and the winner / material / r^2
    gathers go through the caches.  9,001 spheres (2,251 groups) take 71 words of
    the primary pair mask per wave tile, more than the 64 lanes that load them.  RTWeekend's 482 spheres plus small spheres
    scattered over its ground, both rule sets, bit-exact against the oracle."""
    base = rt.scene_builtin(2)
    sp0, _, _ = rt.scene_arrays(base)
    rng = np.random.default_rng(n_spheres)
    extra = sp0[rng.integers(1, len(sp0), n_spheres - len(sp0))].copy()
    extra[:, 0] = rng.uniform(-1.5, 1.5, len(extra))
    extra[:, 2] = rng.uniform(-1.5, 1.5, len(extra))
    extra[:, 4] = rng.uniform(0.004, 0.015, len(extra))
    extra[:, 1] = extra[:, 4]
    sp = np.concatenate([sp0, extra]).astype(np.float32)
    la = (base.LookAt.x, base.LookAt.y, base.LookAt.z)
    kw = dict(distance=base.DefaultDistanceFromLookAt, x_angle=base.DefaultXAngle, y_height=base.DefaultYHeight)
    s = rt.scene_from_spheres(sp, look_at=la, use_sky=True, **kw)
    _, groups, mats = rt.scene_arrays(s)
    assert len(groups) > 265
    o = orc.Scene(sp, groups, mats, look_at=la, use_sky=True, **kw)
    W, H = 40, 24
    cam = rt.camera_setup(s, W, H)
    for simd in (True, False):
        g = gpu_render(rt, torch_cuda, gdev, s, cam, W, H, frames=2, bounces=5, simd=simd)
        r = orc.render(o, orc.camera(o, W, H), W, H, frames=2, max_bounce=5, simd=simd)
        assert_same(*g, *r)


def test_scene_above_the_limit_is_refused(rt, torch_cuda, gdev):
    sp = np.zeros((int(rt.RT_MAX_SPHERES) + 1, 20), np.float32)
    sp[:, 4] = 0.1
    with pytest.raises(rt.RtError, match="exceed"):
        gdev.upload_scene(rt.scene_from_spheres(sp))


@pytest.mark.parametrize("simd", [True, False], ids=["simd", "scalar"])
def test_first_launch_split_changes_no_bit(rt, orc, torch_cuda, simd):
    """The first launch of a key (frames >= 32 P) runs split: a head of 8 samples
    per lane in the cull pass's order, which measures the tile costs, then the
    rest heaviest-first, continuing the running mean (and with SplitParts 3
    a second leading part of 8 per lane).  The frame, the accumulation and the
    ray count equal the unsplit launch's (SplitFirstLaunch off) and the oracle's -- also
    continuing a resident mean (PreviousRayCount > 0) and with
    RT_FLAG_ACCUM_ZERO over a stale buffer."""
    s, o = _scenes(rt, orc, 1, 64)
    W, H, S, B = 192, 128, 128, 8
    cam = rt.camera_setup(s, W, H)
    oc = orc.camera(o, W, H)
    base = orc.render(o, oc, W, H, frames=7, max_bounce=B, threads=orc.cpu_threads())
    cases = [("plain", 0, None, False), ("continued", 7, base[0], False), ("accum_zero", 7, base[0], True)]
    for name, pc, prev0, az in cases:
        out, heads = [], []
        for probe, parts in ((OFF, 2), (ON, 2), (ON, 3)):
            dev = rt.Device(0, options={"LanesPerPixel": 4, "SplitFirstLaunch": probe, "SplitParts": parts,
                                        "SplitGrowth": 1})
            try:
                prev = None if prev0 is None else torch_cuda.from_numpy(prev0.reshape(-1, 4).copy()).cuda()
                out.append(gpu_render(rt, torch_cuda, dev, s, cam, W, H, frames=S, bounces=B, simd=simd,
                                      prev_count=pc, prev=prev, accum_zero=az))
                heads.append(dev.last_info()["SplitHeadFrames"])
            finally:
                dev.close()
        assert heads == [0, 32, 64], (name, heads)
        for g in out[1:]:
            assert torch_cuda.equal(out[0][0], g[0]) and torch_cuda.equal(out[0][1], g[1]) and out[0][2] == g[2], name
        if az or pc == 0:
            r = orc.render(o, oc, W, H, frames=S, max_bounce=B, simd=simd, threads=orc.cpu_threads(),
                           prev_count=pc)
        else:
            r = orc.render(o, oc, W, H, frames=S, max_bounce=B, simd=simd, threads=orc.cpu_threads(),
                           prev_count=pc, prev=base[0])
        assert_same(*out[1], *r)


def test_on_render_resize_returns_no_frame_and_restarts_at_the_new_size(rt, orc, torch_cuda):
    """A call with a different-size image (main.cpp:784-804): it waits for the
    frame in flight, returns 0 and leaves the image alone (CopyToOutput is
    false), restarts the mean, and the next completed frame is frame 0 at the
    new size -- every later one the mean over one more frame.  Within the
    reservation (rt_on_init's 1280x720 window, then rt_on_render_reserve) no
    resize allocates frame buffers."""
    rt.on_init()
    try:
        o = orc.scene_builtin(1)
        allocs0 = rt.on_render_profile()["FrameAllocations"]
        sizes = [(48, 40), (64, 32), (33, 70), (64, 32)]
        for i, (W, H) in enumerate(sizes):
            img = np.full((H, W), 0xDEADBEEF, np.uint32)
            done, rays, _ = rt.on_render(img, 1)  # resize (first call: from no image at all)
            assert not done and rays == 0
            assert np.all(img == 0xDEADBEEF), "a resize must not write the image"
            ocam = orc.camera(o, W, H)
            for k in range(3):
                if i != 1:  # size 1: busy-poll without waiting, like a platform loop
                    rt.on_render_wait()
                while True:
                    done, rays, _ = rt.on_render(img, 1)
                    if done:
                        break
                _, ocur, orays = orc.render(o, ocam, W, H, frames=k + 1, max_bounce=5)
                assert np.array_equal(img.reshape(-1), ocur), (W, H, k)
                assert rays == orc.render(o, ocam, W, H, prev_count=k, frames=1, max_bounce=5)[2], (W, H, k)
        # the mid-loop resize in flight: no wait before it
        W, H = sizes[0]
        img = np.zeros((H, W), np.uint32)
        assert not rt.on_render(img, 1)[0]
        assert rt.on_render_profile()["FrameAllocations"] == allocs0, "a resize within the reservation allocated"
        # beyond the reservation: reserve first, then resize without allocation
        rt.on_render_reserve(1600, 900)
        allocs1 = rt.on_render_profile()["FrameAllocations"]
        assert allocs1 == allocs0 + 1
        for W, H in ((1600, 900), (1500, 800), (96, 64)):
            img = np.zeros((H, W), np.uint32)
            rt.on_render_wait()
            assert not rt.on_render(img, 1)[0]
        rt.on_render_wait()
        assert rt.on_render(img, 1)[0]
        _, ocur, _ = orc.render(o, orc.camera(o, 96, 64), 96, 64, frames=1, max_bounce=5)
        assert np.array_equal(img.reshape(-1), ocur)
        assert rt.on_render_profile()["FrameAllocations"] == allocs1
        rt.on_render_wait()
    finally:
        rt.on_shutdown()


def test_on_render_reset_key_hands_out_the_completed_frame_and_restarts(rt, orc, torch_cuda):
    """R (main.cpp:791-806): the call waits for the frame in flight, copies the
    COMPLETED frame out (returns 1 with that frame), and restarts the mean: the
    next frame handed out is frame 0 again.  Both rule sets; once with the
    frame still in flight at the R call."""
    rt.on_init()
    try:
        W, H = 56, 40
        o = orc.scene_builtin(0)
        ocam = orc.camera(o, W, H)
        want = [orc.render(o, ocam, W, H, frames=k + 1, max_bounce=5)[1] for k in range(4)]
        want_scalar = [orc.render(o, ocam, W, H, frames=k + 1, max_bounce=5, simd=False)[1] for k in range(4)]
        img = np.zeros((H, W), np.uint32)
        for simd, ref in ((True, want), (False, want_scalar)):
            rt.on_render(img, 0, simd, keys=rt.KEY_RESET)  # restart under these rules
            for k in range(3):
                rt.on_render_wait()
                assert rt.on_render(img, 0, simd)[0]
                assert np.array_equal(img.reshape(-1), ref[k]), (simd, k)
            # R while frame 3 may still be in flight: waits, hands out the 4-frame mean
            done, rays, _ = rt.on_render(img, 0, simd, keys=rt.KEY_RESET)
            assert done
            assert np.array_equal(img.reshape(-1), ref[3]), simd
            rt.on_render_wait()
            assert rt.on_render(img, 0, simd)[0]
            assert np.array_equal(img.reshape(-1), ref[0]), simd  # the mean restarted
            rt.on_render_wait()
            assert rt.on_render(img, 0, simd)[0]
            assert np.array_equal(img.reshape(-1), ref[1]), simd
        rt.on_render_wait()
    finally:
        rt.on_shutdown()
