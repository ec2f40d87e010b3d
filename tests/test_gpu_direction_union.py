"""The direction walk's union ("the direction table"; rtk_walk.h wave_or): the OR of the round's
lanes' masks is a fixed reduction that enables every lane of the wave while it runs.

1. rt_direction_union runs that function alone, one wave with a chosen set of lanes enabled, against
   numpy.bitwise_or.reduce over the enabled lanes' words, in both mask widths; every lane's canary register
   must come back unchanged.
2. Sparse rounds through the whole kernel: tiny and ragged frames seen from inside the cloud, so that most of a
   wave's lanes are invalid and every path bounces, bit for bit against the oracle (running mean, RGBA8, rays)."""
import numpy as np
import pytest

from test_gpu_parity import assert_same, gpu_render

pytestmark = pytest.mark.gpu

ROW = 0xFFFF


def lane_masks():
    """The enabled-lane sets the issue names, then 2,000 seeded random ones."""
    named = [1 << l for l in (0, 1, 15, 16, 31, 32, 47, 48, 63)]
    named += [ROW << (16 * r) for r in range(4)]
    named += [(ROW << 16) | (ROW << 48)]                      # rows 1 and 3 only
    named += [0x5555555555555555, 0xAAAAAAAAAAAAAAAA]         # every other lane
    named += [(1 << a) | (1 << b) for a, b in ((0, 3), (12, 19), (31, 32))]  # what a butterfly under partial exec loses
    named += [(1 << 64) - 1]
    rng = np.random.default_rng(2101)
    rand = []
    for k in range(2000):
        density = (0.03, 0.1, 0.5, 0.9)[k % 4]
        bits = rng.random(64) < density
        if not bits.any():
            bits[rng.integers(64)] = True
        rand.append(int(np.bitwise_or.reduce(np.uint64(1) << np.flatnonzero(bits).astype(np.uint64))))
    return named, rand


def sparse_words(rng, dtype):
    """64 words of 0 to 3 bits each (the word 0 on about a quarter of the lanes)."""
    width = 8 * np.dtype(dtype).itemsize
    n_bits = rng.integers(0, 4, 64)
    words = np.zeros(64, dtype)
    for l in range(64):
        for b in rng.integers(0, width, n_bits[l]):
            words[l] |= dtype(1) << dtype(b)
    return words


def expected(words, lanes):
    on = np.array([(lanes >> l) & 1 for l in range(64)], bool)
    return int(np.bitwise_or.reduce(words[on]))


@pytest.fixture(scope="module")
def dev(rt, torch_cuda):
    d = rt.Device(0)
    yield d
    d.close()


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64], ids=["u32", "u64"])
def test_union_of_the_enabled_lanes(rt, dev, dtype):
    named, rand = lane_masks()
    rng = np.random.default_rng(77 + np.dtype(dtype).itemsize)
    # the named sets: every lane a distinct word with a bit of its own where the width allows (u64: bit l),
    # so one missing or one extra lane shows; then the same sets on sparse words
    own = (np.uint64(1) << np.arange(64, dtype=np.uint64)) if dtype is np.uint64 else \
        ((np.uint32(1) << (np.arange(64, dtype=np.uint32) % 32)) | (np.uint32(1) << (np.arange(64, dtype=np.uint32) // 2)))
    own = own.astype(dtype)
    for lanes in named:
        for words in (own, sparse_words(rng, dtype)):
            canary = rng.integers(0, 2**32, 64, dtype=np.uint64).astype(np.uint32)
            got, back = dev.direction_union(words, lanes, canary)
            assert got == expected(words, lanes), (hex(lanes), hex(got), hex(expected(words, lanes)))
            assert np.array_equal(back, canary), (hex(lanes), np.flatnonzero(back != canary).tolist())
    for lanes in rand:
        words = sparse_words(rng, dtype)
        canary = rng.integers(0, 2**32, 64, dtype=np.uint64).astype(np.uint32)
        got, back = dev.direction_union(words, lanes, canary)
        assert got == expected(words, lanes), (hex(lanes), hex(got), hex(expected(words, lanes)), words.tolist())
        assert np.array_equal(back, canary), (hex(lanes), np.flatnonzero(back != canary).tolist())


def test_union_refuses_no_lane_and_other_widths(rt, dev):
    words, canary = np.ones(64, np.uint32), np.zeros(64, np.uint32)
    with pytest.raises(rt.RtError, match="no lane"):
        dev.direction_union(words, 0, canary)
    u, back = np.zeros(2, np.uint32), np.zeros(64, np.uint32)
    assert rt.lib().rt_direction_union(dev.handle, words.ctypes.data, 16, 1, canary.ctypes.data, u.ctypes.data,
                                       back.ctypes.data) == -22
    assert b"MaskBits 16" in rt.lib().rt_last_error()


# ---- sparse rounds through the whole kernel

FRAMES, B = 8, 8
INSIDE = 1.0  # camera distance: inside the cloud, every pixel's paths bounce
SIZES = [(1, 1), (3, 3), (5, 2), (17, 9)]


@pytest.fixture(scope="module")
def inside(rt, orc):
    """Floating Spheres prefixes seen from inside, and the oracle's frames per (n, rule set, size): rendered once."""
    cache = {}

    def get(n, simd, w, h):
        if (n, simd, w, h) not in cache:
            s, o = rt.scene_prefix(rt.scene_builtin(1), n), orc.scene_builtin(1).prefix(n)
            r = orc.render(o, orc.camera(o, w, h, distance=INSIDE), w, h, frames=FRAMES, max_bounce=B, simd=simd)
            r[0].setflags(write=False)
            r[1].setflags(write=False)
            cache[(n, simd, w, h)] = (s, r)
        return cache[(n, simd, w, h)]

    return get


@pytest.mark.parametrize("simd", [True, False], ids=["simd", "scalar"])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("n", [64, 128], ids=["u32_masks", "u64_masks"])
def test_sparse_rounds_give_the_oracle_bits(rt, torch_cuda, inside, n, size, simd):
    w, h = size
    s, ref = inside(n, simd, w, h)
    table, _ = rt.scene_direction_table(s, simd)
    assert table is not None and table.dtype == (np.uint32 if n == 64 else np.uint64)
    for lanes in (4, 8):
        for threshold in (0, 1):  # the default, and rounds of a single lane
            d = rt.Device(0, options={"LanesPerPixel": lanes, "SecondaryThreshold": threshold})
            try:
                g = gpu_render(rt, torch_cuda, d, s, rt.camera_setup(s, w, h, INSIDE), w, h, frames=FRAMES, bounces=B,
                               simd=simd)
                assert_same(*g, *ref)
                info = d.last_info()
                assert info["DirectionTable"] == 1 and info["LanesPerPixel"] == lanes, (lanes, threshold, info)
                assert ref[2] > w * h * FRAMES, "no path bounced"
            finally:
                d.close()
