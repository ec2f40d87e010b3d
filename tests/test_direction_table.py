"""CPU property test of the direction table ("the direction table"; rt_pack.cpp direction_table).

Row j, cell c of rt_scene_direction_table holds bit i >> 1 for every sphere i that a ray leaving ball j in a
direction of cell c can be accepted on.  A lane of the direction walk (rtk_walk.h direction_groups) reads
that mask where it has measured that its origin lies on sphere j (origin_near), and tests only the member
entries of the mask, so a clear bit must be a proven miss: here every sphere the reference-rounded exact test
accepts (test_prefilter_bound.could_accept, main.cpp:401-429 op for op) has its pair bit in the lane's row.

The rays are formed as the reference forms them, with the helpers of test_own_sphere_skip: the reference's
rounded landing on sphere j from a camera or from another sphere (both roots, so origins inside j too), then
new directions -- diffuse, mirror, near-tangent, inward, aimed at another sphere's silhouette from both sides,
and along the 26 axis, edge and corner directions of the cube faces where components tie -- with |D|^2 pushed
to 2^-17 of 1.  The cell function is restated in numpy f32 and compared with the library's own
(rt_direction_cell) on every ray.  The rows of the neighbouring cells are checked too: with every index input
moved by 9e-7 either way (the proof widens a cell's interval by 1e-6; the rest is the f32 rounding of the moved
input), the cell reached must still hold the bit.
"""
import itertools

import numpy as np
import pytest

import random_scenes
from test_own_sphere_skip import OWN_CC, camera_positions, landings, new_directions, stretch
from test_prefilter_bound import could_accept, fma, slot_spheres, unit

F = np.float32
N = 16                                   # rt_layout.h kDirN
SPAN = F(0.7072)                         # kDirSpan
SCALE = F(N) / (F(2.0) * SPAN)           # kDirScale, formed as the header forms it
HALF = F(0.5) * F(N)                     # kDirHalf
CELLS = 6 * N * N
MARGIN = 9e-7

# adversarial scenes (random_scenes.make) that get a one-word scene-wide table with a direction block
ADVERSARIAL = (4010, 4015, 4017, 4022, 4024, 4026, 4038)


def cell_axis(v):
    t = np.floor(fma(v, np.broadcast_to(SCALE, v.shape), np.broadcast_to(HALF, v.shape)))
    return np.clip(t, 0, N - 1).astype(np.int64)


def cell(d):
    """rt_layout.h dir_cell in numpy f32."""
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    ax, ay, az = np.abs(dx), np.abs(dy), np.abs(dz)
    fx = (ax >= ay) & (ax >= az)
    fy = ~fx & (ay >= az)
    m = np.where(fx, dx, np.where(fy, dy, dz))
    a = np.where(fx, dy, dx)
    b = np.where(fx | fy, dz, dy)
    face = np.where(fx, 0, np.where(fy, 2, 4)) + (m < 0)
    return (face * N + cell_axis(a)) * N + cell_axis(b)


def origin_near(cx, cy, cz, rho):
    """rtk_walk.h origin_near: the lane's measurement of the table's origin premise."""
    cc = fma(cx, cx, fma(cy, cy, cz * cz))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(fma(cc, np.broadcast_to(-OWN_CC, cc.shape), rho)) < (rho * F(2.0 ** -6)).astype(F)


LATTICE = np.array([v for v in itertools.product((-1.0, 0.0, 1.0), repeat=3) if any(v)], np.float64)


def more_directions(rng, o, centres, radius, live):
    """Directions aimed at a random sphere's silhouette, half just inside and half just outside its rim, and the
    26 lattice directions (exact ties between components), half of them nudged off the tie."""
    n = len(o)
    i = rng.choice(live, n)
    to = centres[i].astype(np.float64) - o
    w = np.cross(to, rng.normal(size=(n, 3)))
    w /= np.maximum(np.linalg.norm(w, axis=1, keepdims=True), 1e-300)
    aim = 1.0 + rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-7, -1, n)
    sil = stretch(rng, unit(to + w * (radius[i] * aim)[:, None]))
    lat = LATTICE[rng.integers(0, len(LATTICE), n)]
    lat = lat + np.where(rng.random((n, 1)) < 0.5, 0.0, 1.0) * rng.uniform(-1e-6, 1e-6, (n, 3))
    return {"silhouette": sil, "lattice": stretch(rng, unit(lat))}


def check_scene(rt, scene, simd, seed, n=1500):
    """Asserts the table's claim on one rule set; returns (rays that qualify, rays generated)."""
    tab, edge = rt.scene_direction_table(scene, simd)
    assert tab is not None and edge == N and tab.shape[1] == CELLS
    r2, r2p, _ = rt.scene_prefilter(scene, simd)
    rho = rt.scene_own_sphere(scene, simd)
    centres, radius = slot_spheres(rt, scene, simd)
    radius = np.abs(radius).astype(F)
    n_slots = len(r2)
    assert tab.shape[0] == n_slots
    n_pairs = n_slots // 2
    assert tab.dtype == (np.uint32 if n_pairs <= 32 else np.uint64)
    every = np.uint64((1 << n_pairs) - 1)
    tab = tab.astype(np.uint64)
    # own-pair bits always set; a cell no unit direction reaches (both minor components at an end of the
    # grid: a^2 + b^2 ~ 1 leaves no major component) is all-ones
    own_bit = np.uint64(1) << (np.arange(n_slots, dtype=np.uint64) >> np.uint64(1))
    assert np.all(tab & own_bit[:, None] == own_bit[:, None])
    for face in range(6):
        for ia, ib in ((0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1)):
            assert np.all(tab[:, (face * N + ia) * N + ib] == every)
    on = np.isfinite(rho)
    assert np.all(tab[~on] == every), "a row whose lanes cannot measure the premise is not all-ones"
    live = np.flatnonzero((r2 > 0 if simd else r2 >= 0) & np.isfinite(r2) & (radius > 0))
    table_spheres = np.flatnonzero(on)
    rng = np.random.default_rng(seed)
    qualified = generated = 0
    shifts = np.array(list(itertools.product((-MARGIN, MARGIN), repeat=3)))
    # (the scene's own camera and other spheres: landings from the helper's second camera, 200 away with |D|^2 pushed
    # to 2^-17 of 1, lie off the sphere by more than any lane's measurement accepts and would read all-ones rows)
    for src in camera_positions(rt, scene)[:1] + [None, None]:
        j = rng.choice(table_spheres, n)
        if src is None:  # a point on another sphere
            i = rng.choice(live, n)
            prev_o = centres[i].astype(np.float64) + radius[i, None] * unit(rng.normal(size=(n, 3)))
        else:
            prev_o = np.broadcast_to(src, (n, 3)).copy()
        o, dprev, jj, _ = landings(rng, centres, radius, r2, j, prev_o)
        if len(o) == 0:
            continue
        # (a quarter of the origins pushed off the surface, relatively 1e-8 .. 5e-4 either way: inside the premise)
        off = np.where(rng.random((len(o), 1)) < 0.25, 10.0 ** rng.uniform(-8, -3.3, (len(o), 1)), 0.0)
        off *= rng.choice([-1.0, 1.0], (len(o), 1))
        o = (o + ((o - centres[jj]) * off).astype(F)).astype(F)
        kinds = new_directions(rng, o, dprev, centres, jj)
        kinds.update(more_directions(rng, o.astype(np.float64), centres, radius, live))
        near = origin_near(*(centres[jj, k] - o[:, k] for k in range(3)), rho[jj])
        cx, cy, cz = (centres[None, :, k] - o[:, None, k] for k in range(3))
        for kind, d in kinds.items():
            norm_ok = np.abs(1.0 - (d.astype(np.float64) ** 2).sum(1)) <= 2.0 ** -16
            ok = near & norm_ok
            generated += len(d)
            qualified += int(ok.sum())
            c = cell(d)
            lib_c = np.array([rt.direction_cell(*v) for v in d[:: max(1, len(d) // 200)]])
            assert np.array_equal(c[:: max(1, len(d) // 200)], lib_c), f"{kind}: the numpy cell function differs"
            accept = could_accept(cx, cy, cz, d[:, None, 0], d[:, None, 1], d[:, None, 2], r2[None, :], simd)
            need = np.zeros(len(d), np.uint64)
            for s in range(n_slots):
                need |= np.where(accept[:, s], np.uint64(1) << np.uint64(s >> 1), np.uint64(0)).astype(np.uint64)
            rows = tab[jj]
            missing = ok & ((rows[np.arange(len(d)), c] & need) != need)
            assert not np.any(missing), f"{kind}: the lane's row lacks the pair of a sphere it accepts"
            for sh in shifts:
                cn = cell((d.astype(np.float64) + sh).astype(F))
                missing = ok & ((rows[np.arange(len(d)), cn] & need) != need)
                assert not np.any(missing), f"{kind}: a neighbouring cell's row lacks the pair"
            if kind in ("silhouette", "inward"):
                assert np.any(accept[ok] & (np.arange(n_slots)[None, :] != jj[ok, None])), f"{kind}: no ray hits another sphere"
    return qualified, generated


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("n_spheres", [16, 33, 64, 128])
def test_table_holds_every_acceptable_pair_floating_spheres(rt, n_spheres, simd):
    scene = rt.scene_prefix(rt.scene_builtin(1), n_spheres)
    qualified, generated = check_scene(rt, scene, simd, 300 + n_spheres)
    assert generated > 5000 and qualified >= 0.95 * generated, (qualified, generated)


def adversarial_scene(rt, seed):
    spec = random_scenes.make(seed, n_max=300)
    look, dist, ang, yh, _ = spec["cameras"][0]
    return rt.scene_from_spheres(spec["spheres"], look_at=tuple(float(v) for v in look), use_sky=spec["use_sky"],
                                 distance=dist, x_angle=ang, y_height=yh)


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("seed", ADVERSARIAL)
def test_table_on_adversarial_scenes(rt, seed, simd):
    qualified, generated = check_scene(rt, adversarial_scene(rt, seed), simd, 9000 + seed, n=800)
    assert qualified >= 0.95 * generated, (qualified, generated)


def test_adversarial_list_is_every_such_scene(rt):
    """ADVERSARIAL names every scene of the generator's seeds 4000..4039 that gets a direction block."""
    have = tuple(s for s in range(4000, 4040) if rt.scene_direction_table(adversarial_scene(rt, s), True)[0] is not None)
    assert have == ADVERSARIAL


def test_no_table_where_the_fact_cannot_hold(rt):
    """Two-word scenes, per-lane tables, a scene far from its origin (no expanded table in use) and a scene
    without a cluster table have no direction table; the member entries are the expanded table's own."""
    for scene in (rt.scene_prefix(rt.scene_builtin(1), 132), rt.scene_builtin(2), rt.scene_prefix(rt.scene_builtin(1), 4)):
        for simd in (True, False):
            assert rt.scene_direction_table(scene, simd)[0] is None
            assert len(rt.scene_direction_members(scene, simd)) == 0
    sp = rt.scene_arrays(rt.scene_prefix(rt.scene_builtin(1), 64))[0].copy()
    sp[:, 0] += 1e4
    assert rt.scene_direction_table(rt.scene_from_spheres(sp), True)[0] is None
    scene = rt.scene_prefix(rt.scene_builtin(1), 33)
    for simd in (True, False):
        members = rt.scene_direction_members(scene, simd)
        xtab, _, in_use = rt.scene_clusters_expanded(scene, simd)
        n_cpairs = rt.scene_clusters(scene, simd)[1]
        assert in_use and len(members) == 2 * ((33 + 3) // 4)
        seen = set()
        for e in xtab[n_cpairs:].reshape(-1, 16):
            for h in range(2):
                if not np.isfinite(e[6 + h]):
                    continue
                s = int(e[14 + h : 15 + h].view(np.uint32)[0])
                m = members[s >> 1].reshape(16)
                k = s & 1
                assert [m[k], m[2 + k], m[4 + k], m[6 + k], m[12 + k]] == [e[h], e[2 + h], e[4 + h], e[6 + h], e[12 + h]]
                assert m[14 + k : 15 + k].view(np.uint32)[0] == s
                assert np.array_equal(m[8 + 2 * k : 10 + 2 * k].view(np.uint32), e[8 + 2 * h : 10 + 2 * h].view(np.uint32))
                seen.add(s)
        assert seen == set(np.flatnonzero(np.isfinite(rt.scene_prefilter(scene, simd)[1])))  # every sphere of the table
        empty = [s for s in range(len(members) * 2) if s not in seen]
        assert all(np.isneginf(members[s >> 1].reshape(16)[6 + (s & 1)]) for s in empty)
