"""References of the scheduling layer of csrc/rt_sched.hip (test helper): what the heaviest-first tile sort, the XCD
grouping of the wave order and the pixel sort are defined to compute, restated from the comments of that file in
plain numpy and Python integers.  Nothing here follows the kernels' mechanics (ballots, lane walks, block scans):
every function is the definition, computed the slow way.  tests/test_sched_ref.py holds these against brute force,
tests/test_gpu_sched_layer.py holds the kernels of the built library against these."""
import numpy as np

SORT_BUCKETS = 64
REF_TILE = 32  # the reference's TileSize (rt_kernel.h kRefTile)
NOT_PERMUTED = 0xFF

# (TW, TH) of Shape<P> (csrc/rtk_shape.h) for the launch shapes the pixel sort exists for
SHAPES = {4: (4, 4), 8: (4, 2), 16: (2, 2), 32: (2, 1)}


# ------------------------------------------------------------------------------------------------ tile sort
def bucket(c: int) -> int:
    """Quarter-octave bucket of a cost: 0 for cost 0 alone, else 4 log2(c) + the two bits after the leading one,
    offset by 40 and clamped to [1, 63]."""
    c = int(c)
    if c == 0:
        return 0
    l = c.bit_length() - 1
    q = 4 * l + (((c >> (l - 2)) & 3) if l >= 2 else 0) - 40
    return min(max(q, 1), SORT_BUCKETS - 1)


def buckets(cost) -> np.ndarray:
    """bucket() of every element, vectorised (int64)."""
    c = np.asarray(cost, np.uint32).astype(np.int64)
    safe = np.maximum(c, 1)
    # the position of the leading one: float64 holds every u32 exactly, c = f * 2^e with f in [0.5, 1)
    l = np.frexp(safe.astype(np.float64))[1].astype(np.int64) - 1
    frac = np.where(l >= 2, (safe >> np.maximum(l - 2, 0)) & 3, 0)
    q = np.clip(4 * l + frac - 40, 1, SORT_BUCKETS - 1)
    return np.where(c == 0, 0, q)


def tile_order(cost):
    """(order, cost afterwards): descending bucket, ties by ascending index; every cost reset to zero."""
    b = buckets(cost)
    order = np.argsort(-b, kind="stable").astype(np.uint32)
    return order, np.zeros(len(b), np.uint32)


# --------------------------------------------------------------------------------------------- XCD grouping
def xcd_groups(order_in, live_tiles: int):
    """(L, group of every position of [0, L)): first[t] is tile t's least position of the prefix, the tiles that
    have one are ranked by it, and a tile's group is its rank & 7."""
    order_in = [int(u) for u in order_in]
    L = min(len(order_in), 4 * int(live_tiles))
    first = {}
    for i in range(L):
        first.setdefault(order_in[i] >> 2, i)
    grp = {t: r & 7 for r, t in enumerate(sorted(first, key=first.get))}
    return L, [grp[order_in[i] >> 2] for i in range(L)]


def xcd_group(order_in, live_tiles: int) -> np.ndarray:
    """The grouped order: the prefix [0, L) partitioned stably by group, group x's r-th unit at 8r + x while
    r < m (the smallest group's size), the rest behind 8m group by group; [L, n) unchanged."""
    order_in = np.asarray(order_in, np.uint32)
    L, g = xcd_groups(order_in, live_tiles)
    out = order_in.copy()
    members = [[int(order_in[i]) for i in range(L) if g[i] == x] for x in range(8)]
    m = min(len(u) for u in members)
    for x in range(8):
        base = 8 * m + sum(len(members[y]) - m for y in range(x))
        for r, u in enumerate(members[x]):
            out[8 * r + x if r < m else base + (r - m)] = u
    return out


# ----------------------------------------------------------------------------------------------- pixel sort
def pixel_seg(P: int, pix_seg: int) -> int:
    """Pixels per dealt unit: a power of two dividing the block row and the wave's pixels (1, 2 or 4)."""
    TW, TH = SHAPES[P]
    BW, npix = 2 * TW, TW * TH
    if pix_seg >= 4 and npix >= 4 and BW % 4 == 0:
        return 4
    if pix_seg >= 2 and npix >= 2:
        return 2
    return 1


def mask_words(n_groups: int) -> int:
    return (2 * n_groups + 63) // 64


def pixel_perm(P, W, rows, pix_seg, cost, masks=None, n_groups=0, sel=None, prefill=0xEE) -> np.ndarray:
    """The 64 bytes of every block tile after the pixel sort over a table prefilled with `prefill`.
    cost: rows x W u32; masks: (n_tiles, 4, mask_words(n_groups)) u64 or None; sel: the bitmap's u32 words over the
    reference tiles of the image, or None."""
    TW, TH = SHAPES[P]
    BW, BH, NB = 2 * TW, 2 * TH, 4 * TW * TH
    S = pixel_seg(P, pix_seg)
    tiles_x, tiles_y = -(-W // BW), -(-rows // BH)
    sel_tiles_x = -(-W // REF_TILE)
    cost = np.asarray(cost, np.uint32).reshape(rows, W)
    perm = np.full((tiles_x * tiles_y, 64), prefill, np.uint8)
    for tile in range(tiles_x * tiles_y):
        tx, ty = tile % tiles_x, tile // tiles_x
        if sel is not None:
            t = ((ty * BH) // REF_TILE) * sel_tiles_x + (tx * BW) // REF_TILE
            if not (int(sel[t >> 5]) >> (t & 31)) & 1:
                continue
        if masks is not None and any(not np.any(masks[tile, q]) for q in range(4)):
            perm[tile, 0] = NOT_PERMUTED
            continue
        c = []
        for l in range(NB):
            x, y = tx * BW + l % BW, ty * BH + l // BW
            c.append(int(cost[y, x]) if x < W and y < rows else 0)
        seg_cost = [sum(c[s * S:(s + 1) * S]) & 0xFFFFFFFF for s in range(NB // S)]
        ranked = sorted(range(NB // S), key=lambda s: (seg_cost[s], s))
        for rank, s in enumerate(ranked):
            for k in range(S):
                perm[tile, rank * S + k] = s * S + k
    return perm
