"""tests/sched_ref.py against brute force (CPU): the properties the scheduling kernels' comments promise, checked on
the references' outputs without the references' formulas.  tests/test_gpu_sched_layer.py runs the same property
checks (the assert_* functions here) on what the GPU wrote."""
import numpy as np
import pytest

import sched_ref

U32 = np.uint32


# -------------------------------------------------------------------------------------- the property checks
def assert_tile_order(cost, order):
    """A permutation whose buckets never increase and whose equal buckets keep index order."""
    n = len(cost)
    order = np.asarray(order, np.int64)
    assert np.array_equal(np.sort(order), np.arange(n)), "not a permutation"
    b = np.array([sched_ref.bucket(c) for c in cost], np.int64)[order] if n <= 4096 else sched_ref.buckets(cost)[order]
    assert np.all(b[1:] <= b[:-1]), "a heavier bucket follows a lighter one"
    same = b[1:] == b[:-1]
    assert np.all(order[1:][same] > order[:-1][same]), "equal buckets out of index order"


def brute_groups(order_in, live_tiles):
    """(L, {tile: group}) by the definition, tile by tile: the tiles with a unit in the prefix, ordered by the
    least position of any of their units, take groups 0, 1, .., 7, 0, .."""
    order_in = np.asarray(order_in, np.int64)
    L = min(len(order_in), 4 * live_tiles)
    tiles = order_in[:L] >> 2
    firsts = sorted((int(np.flatnonzero(tiles == t)[0]), int(t)) for t in np.unique(tiles))
    return L, {t: k % 8 for k, (_, t) in enumerate(firsts)}


def assert_xcd_group(order_in, out, live_tiles):
    """The four invariants of the grouping: a permutation with [L, n) untouched; every position below 8m holds a
    unit of group p % 8; each group's units keep their input order."""
    order_in, out = np.asarray(order_in, np.int64), np.asarray(out, np.int64)
    L, grp = brute_groups(order_in, live_tiles)
    assert np.array_equal(out[L:], order_in[L:]), "[L, n) changed"
    assert np.array_equal(np.sort(out[:L]), np.sort(order_in[:L])), "the prefix is not a permutation of itself"
    g_in = np.array([grp[int(u) >> 2] for u in order_in[:L]], np.int64)
    g_out = np.array([grp[int(u) >> 2] for u in out[:L]], np.int64)
    m = int(min(np.count_nonzero(g_in == x) for x in range(8)))
    assert np.array_equal(g_out[:8 * m], np.arange(8 * m) % 8), "a position below 8m holds another group's unit"
    for x in range(8):
        assert np.array_equal(out[:L][g_out == x], order_in[:L][g_in == x]), f"group {x} lost its input order"


def assert_pixel_perm(P, W, rows, pix_seg, cost, perm, prefill=0xEE):
    """Every written tile holds a permutation of [0, NB) whose segment costs never decrease; bytes [NB, 64) are never
    written.  Returns the number of written tiles."""
    TW, TH = sched_ref.SHAPES[P]
    BW, BH, NB = 2 * TW, 2 * TH, 4 * TW * TH
    S = sched_ref.pixel_seg(P, pix_seg)
    tiles_x = -(-W // BW)
    cost = np.asarray(cost, U32).reshape(rows, W)
    written = 0
    for tile, row in enumerate(np.asarray(perm, np.uint8).reshape(-1, 64)):
        assert np.all(row[NB:] == prefill), "a byte past the block tile's pixels was written"
        if np.all(row[1:NB] == prefill) and row[0] in (prefill, sched_ref.NOT_PERMUTED):
            continue  # not selected, or marked "not permuted"
        written += 1
        assert np.array_equal(np.sort(row[:NB]), np.arange(NB)), "not a permutation"
        segs = row[:NB].reshape(-1, S).astype(np.int64)
        assert np.all(segs[:, 0] % S == 0) and np.all(np.diff(segs, axis=1) == 1), "a segment was split"
        tx, ty = tile % tiles_x, tile // tiles_x
        x, y = tx * BW + segs % BW, ty * BH + segs // BW
        inside = (x < W) & (y < rows)
        c = np.where(inside, cost[np.minimum(y, rows - 1), np.minimum(x, W - 1)], 0).astype(np.uint64)
        sc = c.sum(axis=1) & np.uint64(0xFFFFFFFF)
        assert np.all(sc[1:] >= sc[:-1]), "segment costs decrease"
        tie = sc[1:] == sc[:-1]
        assert np.all(segs[1:, 0][tie] > segs[:-1, 0][tie]), "equal costs out of index order"
    return written


# ------------------------------------------------------------------------------------------------- bucket
def bucket_edges():
    """Every cost at which the quarter-octave code can change, and its neighbours."""
    v = {0, 1, 2, 3, 2**32 - 1}
    for l in range(1, 32):
        for f in range(4):
            e = ((4 + f) << l) >> 2
            v.update(x for x in (e - 1, e, e + 1) if 0 <= x < 2**32)
    return np.array(sorted(v), np.uint64)


def test_bucket_is_monotone_and_in_range():
    rng = np.random.default_rng(20240611)
    c = np.unique(np.concatenate([bucket_edges(), rng.integers(0, 2**32, 100_000, dtype=np.uint64),
                                  # log-uniform too: uniform values almost never fall below 2^20
                                  np.exp2(rng.uniform(0, 32, 100_000)).astype(np.uint64)]))
    c = c[c < 2**32]
    b = np.array([sched_ref.bucket(int(x)) for x in c])
    assert np.all(np.diff(b) >= 0)
    assert b[0] == 0 and c[0] == 0 and np.all(b[1:] >= 1) and b.max() == 63
    assert set(b.tolist()) == set(range(64)), "a bucket no cost reaches"
    assert np.array_equal(sched_ref.buckets(c.astype(U32)), b), "the vectorised form differs from bucket()"


def test_bucket_resolves_octaves_10_to_25_in_quarters():
    # the comment's claim: 4 log2(c) + the two bits after the leading one, less 40; bucket 1 holds 1 .. 1535
    for l in range(10, 26):
        for f in range(4):
            lo = (4 + f) << (l - 2)
            q = 4 * l + f - 40
            if 1 <= q <= 63:
                assert sched_ref.bucket(lo) == q
            if 2 <= q <= 63:
                assert sched_ref.bucket(lo - 1) == q - 1
    assert sched_ref.bucket(1) == 1 and sched_ref.bucket(1535) == 1 and sched_ref.bucket(1536) == 2
    assert sched_ref.bucket(2**32 - 1) == 63


# ----------------------------------------------------------------------------------------------- tile_order
@pytest.mark.parametrize("n", [1, 2, 65, 1025, 5000])
def test_tile_order_is_a_stable_descending_permutation(n):
    rng = np.random.default_rng(n)
    cost = np.exp2(rng.uniform(0, 32, n)).astype(np.uint64).astype(U32)
    cost[rng.random(n) < 0.3] = 0
    order, after = sched_ref.tile_order(cost)
    assert_tile_order(cost, order)
    assert after.dtype == U32 and len(after) == n and not after.any()


# ------------------------------------------------------------------------------------------------ xcd_group
def sorted_units(n_tiles, live, rng, cut=False):
    """The tile order of a launch's costs: dead tiles four zeros, live tiles four random non-zero costs; cut: some
    live tiles have one zero-cost unit, which sorts behind the live prefix."""
    cost = np.zeros((n_tiles, 4), U32)
    live_ids = rng.permutation(n_tiles)[:min(live, n_tiles)]
    cost[live_ids] = np.exp2(rng.uniform(10, 26, (len(live_ids), 4))).astype(U32)
    if cut and len(live_ids):
        some = live_ids[rng.random(len(live_ids)) < 0.4]
        cost[some, rng.integers(0, 4, len(some))] = 0
    return sched_ref.tile_order(cost.reshape(-1))[0]


XCD_TILES = (1, 7, 8, 9, 255, 256, 257, 1000, 1283)


def xcd_live(n_tiles):
    return sorted({0, 1, 7, 8, 9, n_tiles // 2, n_tiles, n_tiles + 5})


def xcd_inputs(n_tiles, live):
    rng = np.random.default_rng(1000 * n_tiles + live)
    return {"sorted": sorted_units(n_tiles, live, rng), "cut": sorted_units(n_tiles, live, rng, cut=True),
            "random": rng.permutation(4 * n_tiles).astype(U32)}


@pytest.mark.parametrize("n_tiles", [1, 7, 8, 9, 257])
def test_xcd_group_invariants(n_tiles):
    for live in xcd_live(n_tiles):
        for order_in in xcd_inputs(n_tiles, live).values():
            before = order_in.copy()
            out = sched_ref.xcd_group(order_in, live)
            assert np.array_equal(order_in, before)
            assert_xcd_group(order_in, out, live)


def test_xcd_group_small_cases_by_hand():
    # tiles 0..8 live, tile k's units at positions 4k..4k+3, so tile k has rank k and group k & 7
    order_in = np.arange(36, dtype=U32)
    out = sched_ref.xcd_group(order_in, 9)
    # groups 1..7 have 4 units, group 0 has 8 (tiles 0 and 8): m = 4, 32 interleaved, group 0's leftovers last
    assert out.tolist() == [4 * (p % 8) + p // 8 for p in range(32)] + [32, 33, 34, 35]
    # fewer than 8 live tiles: some group is empty, m = 0, the prefix is just partitioned by group
    out = sched_ref.xcd_group(np.array([4, 0, 5, 1, 6, 2, 7, 3], U32), 2)
    assert out.tolist() == [4, 5, 6, 7, 0, 1, 2, 3]
    # a prefix that cuts a tile: L = 4, tile 1 has one unit inside it and is ranked by that one
    out = sched_ref.xcd_group(np.array([0, 1, 2, 4, 3, 5, 6, 7], U32), 1)
    assert out.tolist() == [0, 1, 2, 4, 3, 5, 6, 7]


# ----------------------------------------------------------------------------------------------- pixel_perm
@pytest.mark.parametrize("P", [4, 8, 16, 32])
@pytest.mark.parametrize("pix_seg", [1, 2, 4])
def test_pixel_perm_is_a_cost_ordered_permutation(P, pix_seg):
    W, rows = 37, 19
    rng = np.random.default_rng(P * 10 + pix_seg)
    for cost in (rng.integers(0, 4, (rows, W)).astype(U32), rng.integers(0, 2**30, (rows, W)).astype(U32),
                 rng.integers(2**32 - 8, 2**32, (rows, W), dtype=np.uint64).astype(U32)):
        perm = sched_ref.pixel_perm(P, W, rows, pix_seg, cost)
        TW, TH = sched_ref.SHAPES[P]
        assert perm.shape == (-(-W // (2 * TW)) * -(-rows // (2 * TH)), 64)
        assert assert_pixel_perm(P, W, rows, pix_seg, cost, perm) == len(perm)


def test_pixel_seg_rule():
    assert [sched_ref.pixel_seg(P, s) for P in (4, 8, 16, 32) for s in (1, 2, 4)] == [1, 2, 4] * 3 + [1, 2, 2]


def test_pixel_perm_identity_marks_and_selection():
    P, W, rows = 8, 16, 8
    flat = np.full((rows, W), 7, U32)
    perm = sched_ref.pixel_perm(P, W, rows, 4, flat)
    assert np.array_equal(perm[:, :32], np.tile(np.arange(32, dtype=np.uint8), (len(perm), 1)))
    masks = np.ones((len(perm), 4, 2), np.uint64)
    masks[1, 2] = 0          # tile 1: a quadrant without candidates
    masks[2, :, 0] = 0       # tile 2: candidates in the second word only: still permuted
    perm = sched_ref.pixel_perm(P, W, rows, 4, flat, masks, 33, np.array([1], U32))  # the one reference tile: listed
    assert perm[1].tolist() == [0xFF] + [0xEE] * 63 and perm[2, :32].tolist() == list(range(32))
    perm = sched_ref.pixel_perm(P, W, rows, 4, flat, masks, 33, np.array([0], U32))  # and not listed
    assert np.all(perm == 0xEE)
