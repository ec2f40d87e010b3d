"""CPU property test of the cluster walk's own-sphere rule ("the sphere a ray leaves").

A lane that continues a path from sphere j leaves j out of its own member flags when, with
C = RN(S_j - O), cc = fma |C|^2 and T = fma C.D (rtk_walk.h own_sphere),

    |RN(rho_j - cc (1 - 5 2^-18))| < RN(-T 1.9e-4),        rho_j = r_j^2 or +inf (rt_scene_own_sphere).

That is only allowed if the reference's candidate for j (main.cpp:401-429 / 547-578, restated op for op
in numpy f32 by test_prefilter_bound.could_accept) is rejected whatever the running minima are.  The
rays are formed as the reference forms them: a previous origin (a camera, one of them 200 away, or a
point on another sphere), a direction, the reference-rounded root on sphere j (both roots), the new
origin O = RN(O' + RN(D' t)), and new directions of four kinds -- diffuse, mirror, near-tangent on both
sides of T = 0, inward -- with |D|^2 pushed to 2^-17 of 1.  Origins pushed off the surface are checked
as well: the rule measures rho - cc and assumes nothing about the segment that led to O.
"""
import numpy as np
import pytest

import random_scenes
from test_prefilter_bound import could_accept, fma, slot_spheres, unit

F = np.float32
OWN_CC = F(1.0 - 5.0 * 2.0 ** -18)  # rtk_walk.h kOwnCc
OWN_LAM = F(1.9e-4)                 # rtk_walk.h kOwnLam
R2_MIN, R2_MAX = F(2.6e-6), F(256.0)  # rt_pack.cpp kOwnR2Min / kOwnR2Max
EPS = F(1e-4)


def own_rule(cx, cy, cz, dx, dy, dz, rho):
    """rtk_walk.h own_sphere, lane by lane: True where the lane drops its own sphere."""
    cc = fma(cx, cx, fma(cy, cy, cz * cz))
    T = fma(cz, dz, fma(cy, dy, cx * dx))
    with np.errstate(invalid="ignore", over="ignore"):
        d = fma(cc, np.broadcast_to(-OWN_CC, cc.shape), rho)
        return np.abs(d) < (T * -OWN_LAM).astype(F)


def stretch(rng, d):
    """|D|^2 pushed up to 2^-17 away from 1."""
    d = (d * F(1.0) + d * F(1.0) * rng.uniform(-2 ** -18, 2 ** -18, (len(d), 1)).astype(F)).astype(F)
    assert np.all(np.abs(1.0 - (d.astype(np.float64) ** 2).sum(1)) <= 2 ** -16)
    return d


def landings(rng, centres, radius, r2, j, prev_o):
    """The reference's hit points on sphere j of rays from prev_o aimed into its disc (centre to rim):
    (O, D', j, outside) over both accepted roots, O = RN(O' + RN(D' t))."""
    n = len(j)
    u = unit(rng.normal(size=(n, 3)))
    aim = np.where(rng.random(n) < 0.5, rng.uniform(0, 1, n), 1.0 - 10.0 ** rng.uniform(-7, -1, n))  # (half near the rim)
    to = centres[j].astype(np.float64) - prev_o
    w = np.cross(to, u)
    w /= np.maximum(np.linalg.norm(w, axis=1, keepdims=True), 1e-300)
    d = stretch(rng, unit(to + w * (radius[j] * aim)[:, None]))
    o = prev_o.astype(F)
    cx, cy, cz = (centres[j, k] - o[:, k] for k in range(3))
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    T = (cx * dx + cy * dy) + cz * dz
    qx, qy, qz = cx - dx * T, cy - dy * T, cz - dz * T
    dist = (qx * qx + qy * qy) + qz * qz
    with np.errstate(invalid="ignore"):
        X = np.sqrt((r2[j] - dist).astype(F))
    out = []
    for t, outside in ((T - X, True), (T + X, False)):
        ok = ~(dist > r2[j]) & (t > EPS) & np.isfinite(t)
        tt = t[ok, None]
        out.append(((o[ok] + (d[ok] * tt).astype(F)).astype(F), d[ok], j[ok], np.full(int(ok.sum()), outside)))
    return tuple(np.concatenate(p) for p in zip(*out))


def new_directions(rng, o, dprev, centres, j):
    """Four kinds per landing: diffuse, mirror, near-tangent (both sides of T = 0), inward; the normal
    points away from the centre, and each kind also comes mirrored through the tangent plane (rays
    that continue inside the sphere)."""
    nrm = (o.astype(np.float64) - centres[j].astype(np.float64))
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    n = len(o)
    rnd = unit(rng.normal(size=(n, 3))).astype(np.float64)
    tang = np.cross(nrm, rnd)
    tang /= np.maximum(np.linalg.norm(tang, axis=1, keepdims=True), 1e-300)
    alpha = (10.0 ** rng.uniform(-9, -1, (n, 1))) * rng.choice([-1.0, 1.0], (n, 1))
    dp = dprev.astype(np.float64)
    kinds = {
        "diffuse": nrm + 0.999 * rnd,
        "mirror": dp - 2.0 * (dp * nrm).sum(1, keepdims=True) * nrm,
        "tangent": tang + alpha * nrm,
        "inward": -nrm + 0.9 * rnd,
    }
    out = {}
    for name, v in kinds.items():
        flip = np.where(rng.random((n, 1)) < 0.25, -1.0, 1.0) if name != "tangent" else 1.0
        out[name] = stretch(rng, unit(v - (1.0 - flip) * (v * nrm).sum(1, keepdims=True) * nrm))
    return out


def camera_positions(rt, scene):
    out = []
    for dist in (None, 200.0):
        cam = rt.camera_setup(scene, 64, 64, distance=dist)
        out.append(np.array([cam.CameraPosition.x, cam.CameraPosition.y, cam.CameraPosition.z], np.float64))
    return out


def check_scene(rt, scene, simd, seed, n=3000):
    """Returns (lanes the host's rho lets the rule drop, of lanes tried) over diffuse outward rays;
    asserts the rule against could_accept for the host's rho and for rho = r^2 on every sphere of the
    proven radius range."""
    r2, r2p, _ = rt.scene_prefilter(scene, simd)
    rho = rt.scene_own_sphere(scene, simd)
    centres, radius = slot_spheres(rt, scene, simd)
    radius = np.abs(radius).astype(F)
    assert len(rho) == len(r2)
    in_range = (r2 >= R2_MIN) & (r2 <= R2_MAX)
    on = np.isfinite(rho)
    assert np.all(np.isposinf(rho[~on])) and np.array_equal(rho[on], r2[on]) and not np.any(on & ~in_range)
    assert not np.any(on & ~np.isfinite(r2p)), "the rule is on for a sphere outside the table"
    live = np.flatnonzero((r2 > 0 if simd else r2 >= 0) & np.isfinite(r2) & (radius > 0))
    rng = np.random.default_rng(seed)
    fired = tried = 0
    sources = camera_positions(rt, scene) + [None]
    for src in sources:
        j = rng.choice(live, n)
        if src is None:  # a point on another sphere
            i = rng.choice(live, n)
            prev_o = centres[i].astype(np.float64) + radius[i, None] * unit(rng.normal(size=(n, 3)))
        else:
            prev_o = np.broadcast_to(src, (n, 3)).copy()
        o, dprev, jj, outside = landings(rng, centres, radius, r2, j, prev_o)
        if len(o) == 0:
            continue
        # (a quarter of the origins pushed off the surface, relatively 1e-8 .. 1e-2 either way)
        off = np.where(rng.random((len(o), 1)) < 0.25, 10.0 ** rng.uniform(-8, -2, (len(o), 1)), 0.0)
        off *= rng.choice([-1.0, 1.0], (len(o), 1))
        o = (o + ((o - centres[jj]) * off).astype(F)).astype(F)
        cx, cy, cz = (centres[jj, k] - o[:, k] for k in range(3))
        for kind, d in new_directions(rng, o, dprev, centres, jj).items():
            dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
            accept = could_accept(cx, cy, cz, dx, dy, dz, r2[jj], simd)
            drop_host = own_rule(cx, cy, cz, dx, dy, dz, rho[jj])
            drop_all = own_rule(cx, cy, cz, dx, dy, dz, np.where(in_range[jj], r2[jj], F(np.inf)).astype(F))
            assert not np.any(drop_host & accept), f"{kind}: the rule dropped a sphere its lane can accept"
            assert not np.any(drop_all & accept), f"{kind}: the rule (rho = r^2) dropped a sphere its lane can accept"
            if kind == "tangent":
                assert np.any(accept) or not np.any(in_range[jj]), "no near-tangent ray re-enters its sphere: too tame"
            if kind == "diffuse":
                sel = outside & (off[:, 0] == 0.0) & (((o - centres[jj]) * d).sum(1) > 0)
                fired += int(drop_host[sel].sum())
                tried += int(sel.sum())
    return fired, tried


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("idx,n_spheres", [(1, 64), (1, 256), (0, None), (2, None)])
def test_rule_never_drops_an_acceptable_sphere(rt, idx, n_spheres, simd):
    scene = rt.scene_builtin(idx)
    if n_spheres:
        scene = rt.scene_prefix(scene, n_spheres)
    fired, tried = check_scene(rt, scene, simd, 101 + idx)
    if idx == 1:  # C2's scene (and its 256 spheres): the rule must do its work on diffuse outward rays
        assert tried > 1000 and fired >= 0.5 * tried, (fired, tried)


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("seed", range(20))
def test_rule_on_adversarial_scenes(rt, seed, simd):
    spec = random_scenes.make(4000 + seed, n_max=300)
    look, dist, ang, yh, _ = spec["cameras"][0]
    scene = rt.scene_from_spheres(spec["spheres"], look_at=tuple(float(v) for v in look), use_sky=spec["use_sky"],
                                  distance=dist, x_angle=ang, y_height=yh)
    check_scene(rt, scene, simd, 7000 + seed, n=1200)


def test_rule_is_off_where_nothing_is_proven(rt):
    """RTWeekend's ground sphere (radius 1000; the scene takes per-lane tables), spheres outside the
    radius range, padding slots and scenes without a table: rho = +inf, so no lane ever drops them."""
    rtw = rt.scene_builtin(2)
    for simd in (True, False):
        rho = rt.scene_own_sphere(rtw, simd)
        ground = int(np.argmax(np.abs(slot_spheres(rt, rtw, simd)[1])))
        assert np.isposinf(rho[ground]) and np.all(np.isposinf(rho))
    c2 = rt.scene_prefix(rt.scene_builtin(1), 64)
    for simd in (True, False):
        r2 = rt.scene_prefilter(c2, simd)[0]
        assert np.array_equal(rt.scene_own_sphere(c2, simd), r2), "C2: the rule is on for every sphere"
    sp = rt.scene_arrays(rt.scene_prefix(rt.scene_builtin(1), 16))[0].copy()
    sp[0, 4] = 50.0
    sp[5:9, 4] = 1e-3
    mixed = rt.scene_from_spheres(sp)
    for simd in (True, False):
        rho, r2 = rt.scene_own_sphere(mixed, simd), rt.scene_prefilter(mixed, simd)[0]
        assert np.isposinf(rho[0]) and np.all(np.isposinf(rho[5:9]))
        assert np.all((rho == r2) | np.isposinf(rho))
    pad = rt.scene_prefix(rt.scene_builtin(1), 13)
    assert np.all(np.isposinf(rt.scene_own_sphere(pad, False)[13:]))
    tiny = rt.scene_prefix(rt.scene_builtin(1), 4)  # one group: too few spheres for a table
    assert np.all(np.isposinf(rt.scene_own_sphere(tiny, True)))
    x = np.full(4, F(1.0))
    assert not np.any(own_rule(x * 0, x * 0, x, x * 0, x * 0, -x, np.full(4, F(np.inf))))
