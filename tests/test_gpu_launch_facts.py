"""GPU parity of the launch facts the walk-specialised one-wave kernels take at
compile time (at least one bounce, at least one frame, a non-empty cluster
table) and of the launch-invariant values they test once where they are used
(sky, the accumulation flag, the encode pass, the pixel permutation): the
launches the host routes to the run-time kernel instead, both sides of every
such value, and the weights table's end.  Every case is bit-exact against the
oracle: running mean, RGBA8 and ray count."""
import numpy as np
import pytest

from test_gpu_parity import assert_same, gpu_render

pytestmark = pytest.mark.gpu

# rt_kernel.h kWalk*: the walk compiled into the launched kernel (rt_trace_info.Walk)
WALK_ANY, WALK_CL1 = 0, 2
OFF = -1


@pytest.fixture(scope="module")
def fdev(rt, torch_cuda):
    dev = rt.Device(0)
    yield dev
    dev.close()


@pytest.fixture(scope="module")
def fdev4(rt, torch_cuda):
    """Four lanes per pixel at every frame count.  The walk kernels exist for the launch shapes of
    1 pixel-quad per lane, 4, 8 and 16 lanes per pixel; left to itself the host gives a 2-spp
    launch 2 lanes per pixel, which runs the run-time kernel with the walk dispatched in it
    (rt_trace_info.Walk reports the host's routing in both cases)."""
    dev = rt.Device(0, options={"LanesPerPixel": 4})
    yield dev
    dev.close()


@pytest.fixture(params=["lanes4", "auto"])
def anydev(request, fdev, fdev4):
    """lanes4: the walk-specialised kernel; auto: the same routing on the run-time kernel (2 spp)."""
    return fdev4 if request.param == "lanes4" else fdev


def _builtin(rt, orc, index, n):
    return rt.scene_prefix(rt.scene_builtin(index), n), orc.scene_builtin(index).prefix(n)


def _check(rt, orc, torch, dev, s, o, W, H, spp, B, simd, *, distance=None, prev_count=0, prev_np=None,
           accum_zero=False):
    cam = rt.camera_setup(s, W, H, distance=distance)
    prev = None if prev_np is None else torch.from_numpy(prev_np.copy()).to("cuda")
    g = gpu_render(rt, torch, dev, s, cam, W, H, frames=spp, bounces=B, simd=simd, prev_count=prev_count, prev=prev,
                   accum_zero=accum_zero)
    # (RT_FLAG_ACCUM_ZERO: the running mean so far counts as zero whatever the buffer holds)
    oprev = None if prev_np is None or accum_zero else prev_np.copy()
    r = orc.render(o, orc.camera(o, W, H, distance=distance), W, H, prev_count=prev_count, frames=spp, max_bounce=B,
                   simd=simd, prev=oprev)
    assert_same(*g, *r)
    return g, dev.last_info()


def _random_mean(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 2.0, (n, 4)).astype(np.float32)


def _walk_kernel_ran(info):
    """The launch shape has walk-specialised kernels (rt_kernel.h rtk_walk_shape)."""
    return info["PixelsPerLane"] == 4 or info["LanesPerPixel"] in (4, 8, 16)


@pytest.mark.parametrize("simd", [True, False])
def test_zero_bounces_take_the_run_time_kernel(rt, orc, torch_cuda, anydev, simd):
    """max_bounce = 0 on a scene with a cluster table: the walk kernels hold no zero-bounce
    path, so the launch is routed to the run-time kernel (at four lanes per pixel too, where
    one bounce or more takes a walk kernel); every frame folds black and the ray count is
    the oracle's."""
    s, o = _builtin(rt, orc, 1, 64)
    g, info = _check(rt, orc, torch_cuda, anydev, s, o, 32, 32, 2, 0, simd)
    assert info["ClusteredWalk"] == 1 and info["Walk"] == WALK_ANY, info
    assert float(g[0][:, :3].abs().max()) == 0.0


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("B", [1, 8])
def test_one_and_eight_bounces_take_the_walk_kernel(rt, orc, torch_cuda, anydev, fdev4, B, simd):
    """max_bounce >= 1 is a fact of the walk kernels (B = 1: every sample ends right after
    its first shade); no sky, so their miss path adds nothing."""
    s, o = _builtin(rt, orc, 1, 64)
    _, info = _check(rt, orc, torch_cuda, anydev, s, o, 32, 32, 2, B, simd)
    assert info["ClusteredWalk"] == 1 and info["Walk"] == WALK_CL1, info
    assert _walk_kernel_ran(info) == (anydev is fdev4), info


@pytest.mark.parametrize("simd", [True, False])
def test_sky_on_a_one_word_per_lane_table(rt, orc, torch_cuda, anydev, fdev4, simd):
    """The first 64 spheres of RTWeekend: the sky term on the miss path of a walk kernel."""
    s, o = _builtin(rt, orc, 2, 64)
    assert o.use_sky
    _, info = _check(rt, orc, torch_cuda, anydev, s, o, 32, 32, 2, 8, simd)
    assert info["ClusteredWalk"] == 1 and info["Walk"] != WALK_ANY, info
    assert _walk_kernel_ran(info) == (anydev is fdev4), info


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("accum_zero", [False, True])
def test_one_frame_on_a_running_mean(rt, orc, torch_cuda, fdev, accum_zero, simd):
    """frames = 1 with PreviousRayCount > 0: the load of the mean so far, and the flag that
    skips it (the buffer then holds values that must not be read into the blend)."""
    s, o = _builtin(rt, orc, 1, 64)
    W, H = 32, 32
    _, info = _check(rt, orc, torch_cuda, fdev, s, o, W, H, 1, 8, simd, prev_count=7, prev_np=_random_mean(W * H, 7),
                     accum_zero=accum_zero)
    assert info["Walk"] == WALK_CL1 and _walk_kernel_ran(info), info


@pytest.mark.parametrize("simd", [True, False])
def test_frames_across_the_weights_table_end(rt, orc, torch_cuda, fdev, simd):
    """Eight frames from PreviousRayCount = 65530: the last two lie past the static table of
    the first 65,536 frames' weights."""
    s, o = _builtin(rt, orc, 1, 64)
    W, H = 16, 16
    _, info = _check(rt, orc, torch_cuda, fdev, s, o, W, H, 8, 8, simd, prev_count=65530,
                     prev_np=_random_mean(W * H, 30))
    assert info["Walk"] == WALK_CL1 and _walk_kernel_ran(info), info


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("options", [{}, {"EncodePass": OFF}, {"PixelSort": OFF}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_end_of_kernel_flags(rt, orc, torch_cuda, options, simd):
    """The RGBA8 store left to the encode pass or done by the kernel, and launches with and
    without a pixel permutation (the second launch of a key is the first permuted one)."""
    torch = torch_cuda
    W, H, spp, B = 32, 32, 4, 8
    dev = rt.Device(0, options=options)
    try:
        s, o = _builtin(rt, orc, 1, 64)
        cam = rt.camera_setup(s, W, H)
        r = orc.render(o, orc.camera(o, W, H), W, H, frames=spp, max_bounce=B, simd=simd)
        dev.upload_scene(s)
        sorted_launches = 0
        for _ in range(2):
            prev = torch.full((W * H, 4), float("nan"), device="cuda")
            cur = torch.zeros(W * H, dtype=torch.int32, device="cuda")
            rays = torch.zeros(1, dtype=torch.int64, device="cuda")
            dev.trace(cam, width=W, height=H, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(),
                      rays_ptr=rays.data_ptr(), frames=spp, max_bounce=B, simd=simd, accum_zero=True,
                      stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert_same(prev, cur, int(rays.item()), *r)
            info = dev.last_info()
            assert info["Walk"] == WALK_CL1 and _walk_kernel_ran(info), info
            sorted_launches += info["PixelsSorted"]
        assert sorted_launches == (0 if options.get("PixelSort") == OFF else 1)
    finally:
        dev.close()


@pytest.mark.parametrize("simd", [True, False])
def test_recheck_walk_from_inside_the_cloud(rt, orc, torch_cuda, fdev, simd):
    """The camera inside the 64-sphere cloud: rounds flag the first and the last group of
    the one mask word (bits 0-1 and 30-31) and either or both pairs of a group, which the
    recheck walk's bit tests and mask updates must take in the reference's group order."""
    s, o = _builtin(rt, orc, 1, 64)
    _, info = _check(rt, orc, torch_cuda, fdev, s, o, 64, 48, 4, 8, simd, distance=1.0)
    assert info["Walk"] == WALK_CL1 and _walk_kernel_ran(info), info
