"""The scheduling layer of csrc/rt_sched.hip, each kernel group alone, against exact integer references.

The frame tests cannot see these kernels: any permutation of the tiles renders the same image, their inputs are
measured cycle counts, and the sort zeroes them.  Here the kernels of the built librt_trace.so (tests/sched_probe.py:
the library's own launchers through ctypes, rtk_launch_pixel_sort through tests/sched_probe/libsched_probe.so, which
is linked against the library) run on chosen inputs, and what they wrote is compared with tests/sched_ref.py, the
definitions restated in numpy and Python integers (held against brute force by tests/test_sched_ref.py).  Every
comparison is integer equality.  Every buffer a kernel may write has 64 guard words behind it, checked after the call
(sched_probe.Buf), and every input that must survive is compared with what was sent.

  tile sort      rtk_launch_tile_sort (tile_count / tile_scan / tile_rank, tile_bucket, wave_walk): order equal to the
                 stable descending-bucket order and every cost zeroed, at sizes around the wave, the block, two scan
                 positions per thread, the last size that scans in LDS (256 blocks) and two that scan in global memory
  XCD grouping   rtk_launch_xcd_group (the seven xg_* kernels): equal to the reference, plus the comment's invariants
                 on the GPU output itself; live counts around 8 groups and past n_tiles, prefixes that cut tiles
  pixel sort     pixel_sort_kernel<4, 8, 16, 32> at pix_seg 1, 2, 4 on frames with ragged block tiles: all 64 bytes of
                 every tile, with and without cull masks (one and two words) and a tile selection
  u64 sum        rtk_launch_sum_u64: wrapping sums onto a prefilled destination
  band assembly  rt_assemble_bands where assemble_kernel copies byte by byte: rows that are no multiple of 16 bytes,
                 and 16-byte rows at misaligned pointers

What this cannot see: the costs themselves.  A real launch's tile_cost and pix_cost are cycle counts the trace
kernels measure; whether those are the right thing to sort by is a performance question the benchmark answers.

Measured on an MI355X (profiles/sched_layer_pytest_gpu.log): 191 tests in 4.1 s, all passing on the kernels as they
were: no kernel and no reference had to change.  Three mutations of a scratch copy of rt_sched.hip, one at a time, each
caught here: tile_scan_kernel scanning buckets ascending fails 59 tile-sort cases (every pattern with two buckets in
one launch; the two block patterns from two blocks up); xg_place_kernel without the leftover base fails all 24
grouping cases from 7 tiles up; pixel_sort_kernel without the index tie rule fails all 36 pixel-sort cases.  Each also
broke frames in tests/test_gpu_parity.py (83, 15 and 25 of its 124 tests): the first puts dead tiles in front of the
live prefix, the other two write two units to one slot and so lose one.  What the frames cannot see is a wrong order
that is still a permutation with the live tiles first: that is what the equality with sched_ref holds.
"""
import numpy as np
import pytest

import sched_probe
import sched_ref
from test_sched_ref import (XCD_TILES, assert_pixel_perm, assert_tile_order, assert_xcd_group, xcd_inputs, xcd_live)

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64


@pytest.fixture(scope="module", autouse=True)
def _device(torch_cuda, rt):
    """A HIP device, the package's library loaded, the probe bound to it."""
    sched_probe.libs()


# ------------------------------------------------------------------------------------------------ tile sort
SORT_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 5, 17 * 1024, 256 * 1024, 256 * 1024 + 1, 300 * 1024 + 7)


def bucket_range():
    """least[b], greatest[b]: the least and the greatest cost of every bucket, found by bucket() itself on every
    cost at which the code can change."""
    edges = {0, 1, 2**32 - 1}
    for l in range(2, 32):
        for f in range(4):
            e = (4 + f) << (l - 2)
            edges.update((e - 1, e))
    least, greatest = {}, {}
    for c in sorted(edges):
        b = sched_ref.bucket(c)
        least.setdefault(b, c)
        greatest[b] = c
    assert sorted(least) == list(range(64))
    return np.array([least[b] for b in range(64)], U32), np.array([greatest[b] for b in range(64)], U32)


LEAST, GREATEST = bucket_range()


def _edges(n, rng):
    # every bucket's least and greatest cost in ascending cost order, then 0 1 2 3 and the greatest u32: a sort by raw
    # cost would reverse each bucket's pair, a stable sort by bucket keeps it
    base = np.concatenate([np.stack([LEAST, GREATEST], 1).reshape(-1), np.array([0, 1, 2, 3, 2**32 - 1], U32)])
    return np.resize(base, n)


def _log_uniform(n, rng):
    c = np.exp2(rng.uniform(0, 32, n)).astype(U64).astype(U32)
    c[rng.random(n) < 0.3] = 0
    return c


SORT_PATTERNS = {
    "zero": lambda n, rng: np.zeros(n, U32),
    "one_value": lambda n, rng: np.full(n, 123_456, U32),
    "cull_0_2": lambda n, rng: (2 * rng.integers(0, 2, n)).astype(U32),
    "bucket_edges": _edges,
    "log_uniform": _log_uniform,
    # block j constant: only the cross-block bases order the result
    "blocks_descending": lambda n, rng: LEAST[63 - (np.arange(n) // 1024) % 64],
    "blocks_ascending": lambda n, rng: LEAST[(np.arange(n) // 1024) % 64],
    # every wave's 64 lanes hold 64 distinct buckets (29 is odd), in an order that shifts from wave to wave
    "distinct_per_wave": lambda n, rng: GREATEST[(np.arange(n) * 29 + np.arange(n) // 64) % 64],
}


@pytest.mark.parametrize("pattern", list(SORT_PATTERNS))
@pytest.mark.parametrize("n", SORT_SIZES)
def test_tile_sort(n, pattern):
    cost = SORT_PATTERNS[pattern](n, np.random.default_rng(n))
    assert cost.dtype == U32 and len(cost) == n
    want_order, want_cost = sched_ref.tile_order(cost)
    order, after = sched_probe.tile_sort(cost)
    assert np.array_equal(after, want_cost), f"{np.count_nonzero(after)} costs not zeroed"
    bad = np.flatnonzero(order != want_order)
    assert bad.size == 0, f"{bad.size} of {n} ranks differ, first at {bad[0]}: {order[bad[0]]} for {want_order[bad[0]]}"
    assert_tile_order(cost, order)


# --------------------------------------------------------------------------------------------- XCD grouping
@pytest.mark.parametrize("kind", ["sorted", "cut", "random"])
@pytest.mark.parametrize("n_tiles", XCD_TILES)
def test_xcd_group(n_tiles, kind):
    for live in xcd_live(n_tiles):
        order_in = xcd_inputs(n_tiles, live)[kind]
        want = sched_ref.xcd_group(order_in, live)
        out, in_after = sched_probe.xcd_group(order_in, live)
        assert np.array_equal(in_after, order_in), f"live {live}: the input order changed"
        bad = np.flatnonzero(out != want)
        assert bad.size == 0, (f"live {live}: {bad.size} of {len(out)} positions differ, first at {bad[0]}: "
                               f"{out[bad[0]]} for {want[bad[0]]}")
        assert_xcd_group(order_in, out, live)


def test_xcd_inputs_cut_tiles():
    """The "cut" inputs do what they are for: some live prefix ends inside a tile's four units."""
    cuts = 0
    for n_tiles in XCD_TILES:
        for live in xcd_live(n_tiles):
            order_in = xcd_inputs(n_tiles, live)["cut"]
            L = min(len(order_in), 4 * live)
            inside, outside = set(order_in[:L] >> 2), set(order_in[L:] >> 2)
            cuts += bool(inside & outside)
    assert cuts >= 10


# ----------------------------------------------------------------------------------------------- pixel sort
FRAMES = ((8, 8), (37, 19), (64, 33))
SEL_BITS = 0b0110  # of up to four reference tiles: the first and the last off


def pixel_costs(W, rows, rng):
    i = np.arange(rows * W, dtype=np.int64).reshape(rows, W)
    wrap = np.where(rng.random((rows, W)) < 0.5, 2**32 - 1 - rng.integers(0, 8, (rows, W)), rng.integers(0, 8, (rows, W)))
    return {"equal": np.full((rows, W), 9, U32), "descending": (2**20 - i).astype(U32),
            "ties": rng.integers(0, 4, (rows, W)).astype(U32), "random": rng.integers(0, 2**30, (rows, W)).astype(U32),
            "wrapping": wrap.astype(U32)}


def pixel_masks(n_tiles, n_groups, rng):
    """Cull masks where some tiles have an all-zero quadrant and (two words) some are non-zero in the second alone."""
    nw = sched_ref.mask_words(n_groups)
    masks = rng.integers(1, 2**63, (n_tiles, 4, nw), dtype=np.int64).astype(U64)
    kind = rng.integers(0, 4, n_tiles)
    for t in range(n_tiles):
        if kind[t] == 0:
            masks[t, rng.integers(0, 4)] = 0       # a quadrant without candidates: not permuted
        elif kind[t] == 1 and nw == 2:
            masks[t, :, 0] = 0                     # candidates in the second word alone: permuted
        elif kind[t] == 2 and nw == 2:
            masks[t, rng.integers(0, 4), 1] = 0    # and in the first alone
    if n_tiles >= 2:
        masks[0, 3] = 0
        masks[1, :, 0] = 0 if nw == 2 else masks[1, :, 0]
    return masks


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("pix_seg", [1, 2, 4])
@pytest.mark.parametrize("P", [4, 8, 16, 32])
def test_pixel_sort(P, pix_seg, frame):
    W, rows = frame
    rng = np.random.default_rng(1000 * P + 10 * pix_seg + W)
    TW, TH = sched_ref.SHAPES[P]
    n_tiles = -(-W // (2 * TW)) * -(-rows // (2 * TH))
    sel = np.array([SEL_BITS], U32)
    mask_sets = [(None, 0)] + [(pixel_masks(n_tiles, g, rng), g) for g in (32, 33)]
    for name, cost in pixel_costs(W, rows, rng).items():
        for masks, n_groups in mask_sets:
            for s in (None, sel):
                want = sched_ref.pixel_perm(P, W, rows, pix_seg, cost, masks, n_groups, s)
                got = sched_probe.pixel_sort(P, W, rows, pix_seg, cost, masks, n_groups, s)
                bad = np.flatnonzero((got != want).any(axis=1))
                assert bad.size == 0, (f"{name}, n_groups {n_groups}, sel {s is not None}: {bad.size} of {n_tiles} tiles "
                                       f"differ, first {bad[0]}: {got[bad[0]].tolist()} for {want[bad[0]].tolist()}")
        plain = sched_probe.pixel_sort(P, W, rows, pix_seg, cost)
        assert assert_pixel_perm(P, W, rows, pix_seg, cost, plain) == n_tiles
        if name == "equal" and W % (2 * TW) == 0 and rows % (2 * TH) == 0:
            # nothing to rank by: the identity (a ragged tile's pixels outside the image cost 0 and come first)
            NB = 4 * TW * TH
            assert np.array_equal(plain[:, :NB], np.tile(np.arange(NB, dtype=np.uint8), (n_tiles, 1)))


def test_pixel_sort_cases_reach_every_branch():
    """The inputs above hold what they are for: unselected tiles, marked tiles, tiles live in the second word alone,
    ragged tiles, and segment sums that wrap."""
    W, rows, P = 37, 19, 8
    rng = np.random.default_rng(5)
    n_tiles = 5 * 5
    masks = pixel_masks(n_tiles, 33, rng)
    perm = sched_ref.pixel_perm(P, W, rows, 4, pixel_costs(W, rows, rng)["wrapping"], masks, 33, np.array([SEL_BITS], U32))
    assert np.any(np.all(perm == 0xEE, axis=1)), "no unselected tile"
    assert np.any(perm[:, 0] == 0xFF), "no marked tile"
    second_only = [t for t in range(n_tiles) if not masks[t, :, 0].any() and masks[t, :, 1].all()]
    assert any(perm[t, 0] < 32 for t in second_only), "no tile live in the second mask word alone"
    c = pixel_costs(W, rows, rng)["wrapping"].astype(np.int64)
    assert np.any(c[:, 0:4].sum(axis=1) >= 2**32), "no wrapping segment sum"


# -------------------------------------------------------------------------------------------------- u64 sum
@pytest.mark.parametrize("n", [0, 1, 8, 64])
def test_sum_u64(n):
    rng = np.random.default_rng(n)
    slots = rng.integers(2**63, 2**64, n, dtype=U64)  # any two of them wrap
    slots[::3] = rng.integers(0, 1000, len(slots[::3]), dtype=U64)
    for dst in (0, 0x0123456789ABCDEF, 2**64 - 1):
        want = (dst + sum(int(s) for s in slots)) % 2**64
        assert sched_probe.sum_u64(slots, dst) == want


# -------------------------------------------------------------------------------------------- band assembly
def band_rows_of(height, band_rows, count, rank):
    bands = -(-height // band_rows)
    return sum(min(height, (b + 1) * band_rows) - b * band_rows for b in range(rank, bands, count))


@pytest.mark.parametrize("band_count", [1, 2, 3])
@pytest.mark.parametrize("band_rows", [8, 32])
@pytest.mark.parametrize("layout", ["rows_132B", "rows_144B_off4", "rows_144B_aligned"])
def test_assemble_bands_byte_path(rt, torch_cuda, layout, band_rows, band_count):
    """33 x 70 x 4 B: 132-byte rows; 36 x 70 x 4 B with both pointers 4 bytes off a 16-byte boundary; and the
    latter aligned (the 16-byte path, for contrast).  70 rows: the last band is partial at both band heights."""
    W, H, elem = (33, 70, 4) if layout == "rows_132B" else (36, 70, 4)
    offset = 4 if layout == "rows_144B_off4" else 0
    rng = np.random.default_rng(W * band_rows + band_count)
    rows = [band_rows_of(H, band_rows, band_count, r) for r in range(band_count)]
    assert sum(rows) == H
    max_rows = max(rows)
    src = rng.integers(0, 2**32, (band_count, max_rows, W), dtype=np.int64).astype(U32)
    want = np.empty((H, W), U32)
    for y in range(H):  # the numpy gather: row y lies in band y // band_rows, owned in turn
        band = y // band_rows
        want[y] = src[band % band_count, (band // band_count) * band_rows + y % band_rows]
    d_src, d_dst = sched_probe.Buf(src, offset), sched_probe.Buf(np.full((H, W), 0xDDDDDDDD, U32), offset)
    assert d_src.ptr % 16 == offset and d_dst.ptr % 16 == offset
    rt.assemble_bands(d_src.ptr, max_rows * W * elem, d_dst.ptr, W, H, elem, band_rows, band_count,
                      stream=torch_cuda.cuda.current_stream().cuda_stream)
    torch_cuda.cuda.synchronize()
    assert np.array_equal(d_src.read(), src)
    assert np.array_equal(d_dst.read(), want)
