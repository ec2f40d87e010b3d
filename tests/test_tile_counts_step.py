"""GPU checks of rt_tile_counts_step, the per-tile stopping rule that runs on the device between two
rt_trace_tile_counts calls: random tables and statistics over a 136 x 104 image (20 tiles: one partial pass of
the kernel's block) and a 1920 x 1080 one (2040 tiles: two passes), against the rule restated in numpy.
Integers only, so every comparison is exact.  The edges the rule has are planted in every table: a tile's first
round (PreviousRayCount == 0 never rests on statistics), done == MaxTileFrames, MaxTileFrames - done < done,
Frames > MaxRoundFrames, an entry whose sum does not fit a u32, Frames == 0 (left alone), and a NULL summary."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32 = 0xFFFFFFFF


def effective_frames(prev, frames, max_frames):
    """rt_kernel.h rtk_effective_frames on u32 arrays (int64 arithmetic)."""
    f = np.minimum(frames.astype(np.int64), max_frames)
    return np.where(prev.astype(np.int64) + f > U32, 0, f)


def step_ref(counts, delta, max_round, max_tile, rest_max_delta, rest_sum_squares):
    """The header's rule: ((n, 2) u32 new table, (NextFrames, ActiveTiles, RestedNow))."""
    prev, frames = counts[:, 0].astype(np.int64), counts[:, 1].astype(np.int64)
    f = effective_frames(counts[:, 0], counts[:, 1], max_round)
    ran = f > 0
    done = prev + f
    rest = (done >= max_tile) | ((prev != 0) & (delta[:, 1] <= rest_max_delta) & (delta[:, 3] <= rest_sum_squares))
    nxt = np.where(rest, 0, np.minimum(np.minimum(done, max_round), max_tile - done))
    out = counts.copy()
    out[ran, 0] = done[ran].astype(np.uint32)
    out[ran, 1] = nxt[ran].astype(np.uint32)
    return out, (int(nxt[ran].sum()), int((nxt[ran] > 0).sum()), int((rest & ran).sum()))


def random_input(n, seed, max_round, max_tile, rest_max_delta, rest_sum_squares):
    rng = np.random.default_rng(seed)
    counts = np.stack([rng.integers(0, max_tile + 4, n), rng.integers(0, 2 * max_round + 2, n)], 1).astype(np.uint32)
    delta = np.stack([rng.integers(0, 1025, n), rng.integers(0, 2 * rest_max_delta + 3, n), rng.integers(0, 783361, n),
                      rng.integers(0, 2 * min(rest_sum_squares, 1 << 20) + 3, n)], 1).astype(np.uint32)
    # the planted edges (n >= 20), each beside its neighbour on the other side of the rule
    q = rest_max_delta
    edges = [
        ((0, 4), (9, 0, 9, 0)),                             # first round: never rests on statistics, doubles to 4
        ((4, 4), (9, q, 9, 0)),                             # a later round, MaxDelta at the bound: rests
        ((4, 4), (9, q + 1, 9, 0)),                         # one above: goes on
        ((max_tile - 3, 3), (9, q + 1, 9, 0)),              # done == MaxTileFrames: rests
        ((max_tile - 4, 3), (9, q + 1, 9, 0)),              # done == MaxTileFrames - 1: one frame left
        ((max_tile - 5, 2), (9, q + 1, 9, 0)),              # MaxTileFrames - done (3) < done
        ((2, max_round + 7), (9, q + 1, 9, 0)),             # Frames > MaxRoundFrames: clamped
        ((U32 - 15, max_round), (9, 0, 9, 0)),              # the sum does not fit a u32: left alone
        ((U32 - max_round, max_round), (9, q + 1, 9, 0)),   # it fits exactly: done >= MaxTileFrames, rests
        ((7, 0), (9, 0, 9, 0)),                             # Frames == 0: left alone, statistics or not
        ((0, 0), (0, 0, 0, 0)),
        ((max_tile + 9, 1), (9, q + 1, 9, 0)),              # already past MaxTileFrames: one more round, then rests
        ((5, 5), (9, q, 9, rest_sum_squares + 1 if rest_sum_squares != U32 else U32)),  # SumSquares over the bound / at it
        ((5, 5), (9, q, 9, rest_sum_squares)),
    ]
    at = rng.permutation(n)[:len(edges)]
    for i, (c, d) in zip(at, edges):
        counts[i], delta[i] = c, d
    return counts, delta


RULES = [(16, 32, 1, U32), (16, 32, 3, 5000), (1, 7, 0, U32), (64, 4096, 2, 1 << 20), (U32, U32, 255, U32)]


@pytest.mark.parametrize("size", [(136, 104), (1920, 1080)], ids=["136x104", "1920x1080"])
@pytest.mark.parametrize("rule", RULES, ids=[f"round{r[0]}_tile{r[1]}_d{r[2]}_s{r[3]}" for r in RULES])
def test_step_matches_the_rule(rt, torch_cuda, size, rule):
    check_the_numpy_rule_on_entries_known_by_hand()
    torch = torch_cuda
    w, h = size
    n = rt.tile_count(w, h)
    assert n == {(136, 104): 20, (1920, 1080): 2040}[size]
    mr, mt = rule[0], rule[1]
    counts, delta = random_input(n, 11 + n, min(mr, 1 << 16), min(mt, 1 << 20), rule[2], rule[3])
    want, want_summary = step_ref(counts, delta, *rule)
    assert (want != counts).any() and want_summary[1] > 0 and want_summary[2] > 0  # (the input exercises the rule)
    d_counts = torch.from_numpy(counts.view(np.int32).copy()).to("cuda")
    d_delta = torch.from_numpy(delta.view(np.int32).copy()).to("cuda")
    d_summary = torch.full((4,), -1, dtype=torch.int32, device="cuda")  # (poisoned: written, never accumulated)
    stream = torch.cuda.current_stream().cuda_stream
    r = rt.tile_rule(*rule)
    rt.tile_counts_step(d_counts.data_ptr(), d_delta.data_ptr(), w, h, r, d_summary.data_ptr(), stream)
    torch.cuda.synchronize()
    got = d_counts.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (bad[:8], counts[bad[:8]].tolist(), delta[bad[:8]].tolist(), got[bad[:8]].tolist(),
                           want[bad[:8]].tolist())
    s = d_summary.cpu().numpy().view(rt.tile_step_summary_dtype)[0]
    print("summary", s, "expected", want_summary)
    assert (int(s["NextFrames"]), int(s["ActiveTiles"]), int(s["RestedNow"])) == want_summary
    assert np.array_equal(d_delta.cpu().numpy().view(np.uint32), delta)  # (the statistics are read only)
    # a second step on the result, without a summary: the same table as the rule gives, nothing else written
    want2, _ = step_ref(want, delta, *rule)
    rt.tile_counts_step(d_counts.data_ptr(), d_delta.data_ptr(), w, h, r, 0, stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_counts.cpu().numpy().view(np.uint32), want2)
    assert d_summary.cpu().numpy().tobytes() == s.tobytes()


def check_the_numpy_rule_on_entries_known_by_hand():
    """The restatement itself, on entries whose outcome is known by hand: {done, rest ? 0 : min(done, MaxRoundFrames,
    MaxTileFrames - done)}, a first round never at rest on its statistics."""
    c = np.array([[0, 2], [2, 2], [4, 4], [8, 8], [16, 16], [24, 8], [4, 4], [0, 100], [U32 - 15, 32], [9, 0]], np.uint32)
    d = np.zeros((10, 4), np.uint32)
    d[:, 1] = 5
    d[6, 1] = 1  # the one tile whose statistics are at rest
    out, summary = step_ref(c, d, 16, 32, 1, U32)
    assert out.tolist() == [[2, 2], [4, 4], [8, 8], [16, 16], [32, 0], [32, 0], [8, 0], [16, 16], [U32 - 15, 32], [9, 0]]
    assert summary == (2 + 4 + 8 + 16 + 16, 5, 3)
