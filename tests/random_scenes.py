"""Seeded adversarial scenes for the proof-based skips (test helper).

The kernel skips work by proofs that rest on host-derived error bounds: the
f64 primary-ray cone cull, the FMA secondary-ray prefilter, the cluster walk
and its behind-origin rule.  The built-in scenes exercise them
only in one regime, so this generator builds scenes that stress the slack:
- sphere counts from 1 to 1,060 (265 groups; the four-wave kernels' LDS image holds up to 164);
- radii log-uniform over 1e-3 ... 1e2 of a world scale itself drawn from
  1e-2 ... 1e2 (so the reference's absolute eps = 1e-4 is met at every scale),
  or, in "cloud" scenes, within one decade (the scene-wide prefilter bound
  then pays, and the cluster walk runs);
- overlapping, nested, near-coincident and near-tangent sphere pairs;
- four cameras per scene: outside the cloud, inside a sphere, on a sphere's
  surface, and one with spheres placed tangent to film rays (grazing hits);
- random materials: diffuse, specular, dielectric (IOR < 1 and > 1), emissive,
  with and without the sky term.
Scenes are rt_scalar_sphere records (main.cpp:17-21) converted to groups as
ConvertScalarSpheresToSIMDSpheres does (rt.scene_from_spheres).
Beside the seeds, `named` gives sized and derived inputs for the regimes no seed draws (SIZED, "tiny")."""
import numpy as np

F = np.float32


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _camera_pos(look, distance, x_angle, y_height):
    return np.array([np.cos(x_angle) * distance + look[0], y_height + look[1], np.sin(x_angle) * distance + look[2]])


def make(seed: int, n_max: int = 1060, *, n: int = None, cloud: bool = None):
    """Returns dict(spheres (N,20) f32, use_sky, cameras=[(look_at, distance, x_angle, y_height, kind)]).
    n and cloud, where given, replace the seed's own sphere count and its cloud/wide choice: the
    seed's draws for both are still consumed, so every later stream (positions, adversarial pairs,
    materials, cameras) is drawn in the same order, and a seed without overrides keeps every byte
    (tests/golden/random_scene_digests.json)."""
    rng = np.random.default_rng(seed)
    scale = float(10.0 ** rng.uniform(-2, 2))
    # "cloud" scenes (radii within one decade, like the built-in Floating Spheres)
    # keep the scene-wide prefilter bound useful, so the cluster walk and its
    # behind-origin rule run; "wide" scenes (radii over three decades, a huge
    # sphere) take the per-lane thresholds
    drawn_cloud = rng.random() < 0.4
    if drawn_cloud:
        drawn_n = int(rng.integers(8, 257))
    else:  # mostly small scenes (fast oracle), some large, one in ten at the maximum
        drawn_n = int(rng.choice([rng.integers(1, 9), rng.integers(9, 80), rng.integers(80, 300), n_max],
                                 p=[0.25, 0.45, 0.2, 0.1]))
    cloud = drawn_cloud if cloud is None else bool(cloud)
    n = drawn_n if n is None else int(n)
    extent = scale * rng.uniform(1.0, 4.0)
    c = rng.uniform(-extent, extent, (n, 3))
    r = scale * (10.0 ** rng.uniform(np.log10(0.05), np.log10(0.3), n) if cloud else 10.0 ** rng.uniform(-3, 0, n))
    if not cloud and n > 4 and rng.random() < 0.3:  # one huge sphere (a ground, or a sphere around everything)
        k = rng.integers(n)
        r[k] = scale * 10.0 ** rng.uniform(1, 2)
        if rng.random() < 0.5:
            c[k] = [0.0, -r[k] - scale * 0.5, 0.0]
    # adversarial pairs: tangent (outside / inside), near-coincident, nested
    for i in range(1, n):
        u = rng.random()
        if u < 0.12:
            d = _unit(rng.normal(size=3))
            c[i] = c[i - 1] + d * (r[i - 1] + r[i]) * (1.0 + rng.uniform(-1e-6, 1e-6))
        elif u < 0.18:
            d = _unit(rng.normal(size=3))
            big, small = max(r[i - 1], r[i]), min(r[i - 1], r[i])
            r[i - 1], r[i] = big, small
            c[i] = c[i - 1] + d * (big - small) * (1.0 - rng.uniform(0, 1e-6))
        elif u < 0.22:
            c[i] = c[i - 1] * (1.0 + rng.uniform(-1e-7, 1e-7, 3))
            r[i] = r[i - 1] * (1.0 + rng.uniform(-1e-7, 1e-7))
        elif u < 0.26:
            c[i] = c[i - 1] + rng.uniform(-0.5, 0.5, 3) * r[i - 1]
    sp = np.zeros((n, 20), F)
    sp[:, 0:3] = c
    sp[:, 4] = r
    for i in range(n):
        m = sp[i, 8:20]  # Color(4) Emissive(4) Specular IOR pad pad
        m[0:3] = rng.uniform(0.05, 1.0, 3)
        kind = rng.random()
        if kind < 0.15:
            m[9] = rng.choice([1.5, 1.33, 2.4, 1.0 / 1.5])
        elif kind < 0.4:
            m[8] = rng.uniform(0.0, 1.0)
        if rng.random() < 0.1:
            m[4:7] = rng.uniform(0.0, 4.0, 3)
    use_sky = bool(rng.random() < 0.5)
    centroid = c.mean(0)
    cams = [(centroid, float(extent * rng.uniform(2.0, 4.0)), float(rng.uniform(-6, 6)),
             float(extent * rng.uniform(-0.5, 0.5)), "outside")]
    k = int(np.argmax(r))
    cams.append((c[k], float(r[k] * rng.uniform(0.1, 0.8)), float(rng.uniform(-6, 6)), 0.0, "inside"))
    k = rng.integers(n)
    ang = float(rng.uniform(-6, 6))
    cams.append((c[k], float(np.float32(r[k])), ang, 0.0, "on_surface"))
    cams.append((centroid, float(extent * rng.uniform(1.5, 3.0)), float(rng.uniform(-6, 6)),
                 float(extent * rng.uniform(-0.3, 0.3)), "grazing"))
    return {"spheres": sp, "use_sky": use_sky, "cameras": cams, "scale": scale, "n": n, "cloud": cloud}


# Sized and derived inputs beside the seeds, for the regimes no seed draws (checked on the CPU by
# tests/test_random_scene_inputs.py, traced by tests/test_gpu_random_scene_kernels.py).  Group counts are
# those of the bare scene / with the four grazing spheres the GPU tests add.
SIZED = {
    "wide400": dict(seed=18, n=400, cloud=False),    # 100 / 101 groups: a two-level per-lane table of four mask words
    "wide130": dict(seed=18, n=520, cloud=False),    # 130 / 131 groups: the first size past the cluster table's 128
    "cloud130": dict(seed=6, n=520, cloud=True),
    "wide165": dict(seed=18, n=660, cloud=False),    # 165 / 166 groups: past the four-wave kernels' LDS image (164)
    "cloud165": dict(seed=6, n=660, cloud=True),
    "cloud2w": dict(seed=6, n=200, cloud=True),      # 50 / 51 groups: a scene-wide table of two mask words
    "cloud4w": dict(seed=6, n=400, cloud=True),      # 100 / 101 groups: a scene-wide table of four mask words
}
TINY_SEED, TINY_RADIUS = 34, 2e-6
NAMED = ("tiny",) + tuple(SIZED)
SEED_NAMES = tuple(f"seed{s}" for s in range(56))
# The inputs the forced device options run on: a scene of <= 2 groups (merged rounds), a small wide scene, a wide
# scene with a huge sphere, a one-level and a two-level cloud, 265 groups, tiny, both 130- and 165-group pairs,
# and the two four-word tables (each property checked by tests/test_random_scene_inputs.py)
OPTION_INPUTS = ("seed29", "seed1", "seed16", "seed3", "seed31", "seed18", "tiny", "wide130", "cloud130",
                 "wide165", "cloud165", "cloud4w", "wide400")


def named(name: str):
    """(spec, seed of its grazing spheres) of an input by name: "seed<k>" is make(k) as it is; a SIZED
    name is its seed with the sphere count and the cloud/wide choice fixed; "tiny" is seed 34's spheres
    with the smallest radius set to 2e-6, so that r^2 = 4e-12 lies below 2^-36, the short square
    root's proven range (the host must clear that flag and route the run-time kernel)."""
    if name.startswith("seed"):
        seed = int(name[4:])
        return make(seed), seed
    if name == "tiny":
        spec = make(TINY_SEED)
        sp = spec["spheres"].copy()
        sp[int(np.argmin(sp[:, 4])), 4] = F(TINY_RADIUS)
        spec["spheres"] = sp
        return spec, TINY_SEED
    return make(**SIZED[name]), SIZED[name]["seed"]


def add_grazing_spheres(rt, spec, W, H, count=4, seed=0):
    """Spheres tangent to film rays of the 'grazing' camera (distance from the
    pixel-centre ray = r (1 +- 1e-6)): returns a new spheres array."""
    rng = np.random.default_rng(seed)
    look, dist, ang, yh, _ = spec["cameras"][3]
    tmp = rt.scene_from_spheres(spec["spheres"], look_at=tuple(look), distance=dist, x_angle=ang, y_height=yh)
    cam = rt.camera_setup(tmp, W, H)
    v = lambda a: np.array([a.x, a.y, a.z], np.float64)
    cp, cx, cy, fc = v(cam.CameraPosition), v(cam.CameraX), v(cam.CameraY), v(cam.FilmCenter)
    extra = []
    for _ in range(count):
        x, y = rng.uniform(0, W), rng.uniform(0, H)
        ka = (-1.0 + 2.0 * x / W) * cam.FilmW * 0.5
        kb = (-1.0 + 2.0 * y / H) * cam.FilmH * 0.5
        d = _unit(fc - cp + ka * cx + kb * cy)
        t = spec["scale"] * rng.uniform(0.5, 3.0)
        rad = spec["scale"] * 10.0 ** rng.uniform(-2, -0.5)
        nrm = _unit(np.cross(d, rng.normal(size=3)))
        row = np.zeros(20, F)
        row[0:3] = cp + d * t + nrm * rad * (1.0 + rng.uniform(-1e-6, 1e-6))
        row[4] = rad
        row[8:11] = rng.uniform(0.1, 1.0, 3)
        extra.append(row)
    return np.concatenate([spec["spheres"], np.array(extra, F)])[: 4 * 265]


def build(rt, orc, spheres, use_sky, look, distance, x_angle, y_height):
    """(rt scene, oracle scene) sharing one sphere array and look-at point."""
    s = rt.scene_from_spheres(spheres, look_at=tuple(float(v) for v in look), use_sky=use_sky, distance=distance,
                              x_angle=x_angle, y_height=y_height)
    sp, groups, mats = rt.scene_arrays(s)
    o = orc.Scene(sp, groups, mats, look_at=tuple(float(v) for v in look), use_sky=use_sky, distance=distance,
                  x_angle=x_angle, y_height=y_height)
    return s, o
