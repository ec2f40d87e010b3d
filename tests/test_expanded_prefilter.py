"""CPU property test of the expanded prefilter of the scene-wide cluster walks (DESIGN.md §3,
"the expanded prefilter"; rtk_walk.h pair_prefilter_x; rt_pack.cpp expand_table).

The walk-specialised kernels test a cluster or member pair in 7 packed FMAs on the recentred table
of rt_scene_clusters_expanded: with S' from the table and O' = RN(O - c0),
  T  = fma(S'x, Dx, fma(S'y, Dy, fma(S'z, Dz, -O'.D)))
  A  = fma(S'x, -2O'x, fma(S'y, -2O'y, fma(S'z, -2O'z, |O'|^2)))
  e' = fma(-T, T, A)
and skip on e' >= t' (near the line) or T < b' (behind).  This restates that in numpy f32 and checks,
on the rays the bound is meant for, that nothing skipped holds a sphere the reference-rounded exact
test (test_prefilter_bound.could_accept) accepts, that the table covers every hittable sphere once,
that the form still culls, and that a scene far from its own coordinates' origin turns it off.
"""
import numpy as np
import pytest

import random_scenes
from test_prefilter_bound import could_accept, exact_dist, fma, prefilter, rays, slot_spheres

F = np.float32
N_RAYS = 4000


def translated(rt, scene, dx):
    """The scene with every sphere moved by dx along x."""
    sp, _, _ = rt.scene_arrays(scene)
    sp = sp.copy()
    sp[:, 0] += F(dx)
    return rt.scene_from_spheres(sp)


def decode(rt, scene, simd):
    """The expanded table's clusters and members: ([(entry, half, member slots under it)] over both
    levels, {slot: (member entry, half)}), with the rows the expanded form must not change compared
    against the plain table."""
    tab, ncp = rt.scene_clusters(scene, simd)
    xtab, c0, use = rt.scene_clusters_expanded(scene, simd)
    assert xtab.shape == tab.shape and ncp > 0
    assert np.array_equal(xtab[:, 2].view(np.uint32), tab[:, 2].view(np.uint32)), "ranges / word-0 bits changed"
    assert np.array_equal(xtab[:, 3, 2:].view(np.uint32), tab[:, 3, 2:].view(np.uint32)), "slots changed"
    assert np.array_equal(xtab[:, 4:].view(np.uint32), tab[:, 4:].view(np.uint32)), "bit rows changed"
    assert np.array_equal(np.isneginf(xtab[:, 1, 2:]), np.isneginf(tab[:, 1, 2:])), "padding changed"
    levels, n_sub = rt.scene_cluster_layout(scene, simd)
    clusters, member_of = [], {}

    def members(first, count):
        ms = []
        for m in range(first, first + count):
            for w in range(2):
                if np.isneginf(xtab[m, 1, 2 + w]):
                    continue
                s = int(xtab[m, 3].view(np.uint32)[2 + w])
                assert s not in member_of, "a sphere is a member twice"
                member_of[s] = (m, w)
                ms.append(s)
        return ms

    for c in range(ncp):
        u = xtab[c, 2].view(np.uint32)
        for h in range(2):
            first, count = int(u[2 * h]), int(u[2 * h + 1])
            if levels == 2:
                under = []
                for e in range(first, first + count):
                    assert ncp <= e < ncp + n_sub
                    us = xtab[e, 2].view(np.uint32)
                    for h2 in range(2):
                        ms = members(int(us[2 * h2]), int(us[2 * h2 + 1]))
                        clusters.append((e, h2, ms))
                        under += ms
                clusters.append((c, h, under))
            else:
                clusters.append((c, h, members(first, count)))
    return tab, xtab, c0, use, clusters, member_of


def expanded(xtab, c0, o, d, entry, half):
    """(near-line skip, behind skip, T) of table entries `entry` / halves `half` (arrays) for rays o, d:
    the kernel's ops in the kernel's order (rtk_walk.h ray_expand, pair_prefilter_x)."""
    ox, oy, oz = ((o[:, k] - c0[k]).astype(F)[:, None] for k in range(3))
    dx, dy, dz = (d[:, k][:, None] for k in range(3))
    oo = fma(ox, ox, fma(oy, oy, oz * oz))
    nod = -fma(ox, dx, fma(oy, dy, oz * dz))
    sx, sy, sz = (np.broadcast_to(xtab[entry, r, 2 * q + half][None, :], (len(o), len(entry)))
                  for r, q in ((0, 0), (0, 1), (1, 0)))
    bc = lambda v: np.broadcast_to(v, sx.shape)
    T = fma(sx, bc(dx), fma(sy, bc(dy), fma(sz, bc(dz), bc(nod))))
    A = fma(sx, bc(F(-2) * ox), fma(sy, bc(F(-2) * oy), fma(sz, bc(F(-2) * oz), bc(oo))))
    e = fma(-T, T, A)
    with np.errstate(invalid="ignore"):
        near = e >= xtab[entry, 1, 2 + half][None, :]
        behind = T < xtab[entry, 3, half][None, :]
    return near, behind, T


def check_expanded(rt, scene, simd, seed, require_culls):
    """Returns (in use, member pairs flagged by the expanded form, by the 10-op form) over the rays."""
    tab, xtab, c0, use, clusters, member_of = decode(rt, scene, simd)
    r2, r2p, flags = rt.scene_prefilter(scene, simd)
    assert not flags & 4
    centres, radius = slot_spheres(rt, scene, simd)
    live = np.isfinite(r2p)
    assert sorted(member_of) == sorted(np.flatnonzero(live)), "every hittable sphere is a member exactly once"
    if use:
        assert np.all(np.isfinite(c0)) and np.all(np.isfinite(xtab[:, :2][~np.isneginf(xtab[:, :2])]))
    rng = np.random.default_rng(seed)
    o, d = rays(rng, centres[live], np.abs(radius[live]).astype(F), N_RAYS)
    cx = centres[None, :, 0] - o[:, None, 0]
    cy = centres[None, :, 1] - o[:, None, 1]
    cz = centres[None, :, 2] - o[:, None, 2]
    dx, dy, dz = d[:, None, 0], d[:, None, 1], d[:, None, 2]
    accept = could_accept(cx, cy, cz, dx, dy, dz, r2[None, :], simd) & live[None, :]
    slots = np.array(sorted(member_of))
    ent = np.array([member_of[s][0] for s in slots])
    half = np.array([member_of[s][1] for s in slots])
    near, behind, _ = expanded(xtab, c0, o, d, ent, half)
    assert not np.any(accept[:, slots] & (near | behind)), "the member test skipped a sphere a lane can accept"
    for e, h, ms in clusters:
        if np.isneginf(xtab[e, 1, 2 + h]):
            assert not ms
            continue
        nc, bc, _ = expanded(xtab, c0, o, d, np.array([e]), np.array([h]))
        skip = (nc | bc)[:, 0]
        assert not np.any(accept[skip][:, ms]), "a skipped cluster holds a sphere a lane can accept"
    # the 10-op form on the plain table, for the ratio of flagged member pairs
    e_s, t_s = prefilter(cx, cy, cz, dx, dy, dz, with_t=True)
    old_flag = (e_s[:, slots] < tab[ent, 1, 2 + half][None, :]) & ~(t_s[:, slots] < tab[ent, 3, half][None, :])
    new_flag = ~near & ~behind
    if require_culls:
        # the project's own criterion (test_prefilter_bound.check_prefilter), on the near-line rule alone
        dist = exact_dist(cx, cy, cz, dx, dy, dz)
        hit = ((dist < r2) if simd else ~(dist > r2)) & live[None, :]
        assert hit.sum() > 0
        assert (~near).sum() < 1.5 * hit.sum() + 0.05 * hit.size
    return use, int(new_flag.sum()), int(old_flag.sum())


@pytest.mark.parametrize("n_spheres", [16, 37, 64, 100, 256])
@pytest.mark.parametrize("simd", [True, False])
def test_expanded_prefilter_never_skips_an_exact_hit(rt, n_spheres, simd):
    scene = rt.scene_prefix(rt.scene_builtin(1), n_spheres)
    use, new, old = check_expanded(rt, scene, simd, 23 + n_spheres, require_culls=True)
    assert use, "Floating Spheres runs the walk-specialised kernels"
    print(f"flagged member pairs, {n_spheres} spheres simd={simd}: expanded {new} / 10-op {old} = {new / max(old, 1):.4f}")


@pytest.mark.parametrize("seed", range(40))
def test_expanded_prefilter_on_random_scenes(rt, orc, seed):
    spec = random_scenes.make(seed)
    look, dist, ang, yh, _ = spec["cameras"][0]
    scene, _ = random_scenes.build(rt, orc, spec["spheres"], spec["use_sky"], look, dist, ang, yh)
    for simd in (True, False):
        if rt.scene_clusters_expanded(scene, simd)[0].shape[0] == 0:
            continue  # no scene-wide table (none at all, or per-lane thresholds)
        check_expanded(rt, scene, simd, seed, require_culls=False)


def test_scene_far_from_its_origin_is_not_in_use(rt):
    scene = rt.scene_prefix(rt.scene_builtin(1), 64)
    far = translated(rt, scene, 1e4)
    for simd in (True, False):
        assert rt.scene_clusters_expanded(scene, simd)[2]
        xtab, c0, use = rt.scene_clusters_expanded(far, simd)
        assert xtab.shape[0] > 0 and not use
