"""numpy restatements of the walk layer (csrc/rtk_walk.h), lane by lane and op for op in f32: what
tests/walk_probe computes on the device must equal these bit for bit (tests/test_gpu_walk_layer.py), and
tests/test_walk_ref.py holds them to something else on the CPU (rational arithmetic, the oracle's own group test,
plain per-lane loops written from the reference's text).

Every array is f32 and every f32 operation of the kernel is one numpy f32 operation here, so each rounds once as the
kernel's does (the kernel units are built with -ffp-contract=off and IEEE denormals).  The one fused operation is
`fma` below, which is correctly rounded.
"""
import numpy as np

F = np.float32
U = np.uint32

EPS = F(1e-4)    # rtk_math.h kEps
FMAX = F(1e30)   # rtk_math.h kFMax
KEY_INSIDE = U(0x80000000)  # rtk_walk.h kKeyInside
OWN_NONE = U(0xFFFFFFFF)    # rtk_walk.h kOwnNone
PF_REL = F(2.0 ** -15)             # rtk_walk.h kPfRel
CL_REL = F(9.2e-4)                 # rtk_walk.h kClRel
BEHIND_REL = F(4.5 * 2.0 ** -24)   # rtk_walk.h kBehindRel
SLAB_REL = F(2.0 ** -9)            # rt_layout.h kSlabRel
OWN_CC = F(1.0 - 5.0 * 2.0 ** -18)  # rtk_walk.h kOwnCc
OWN_LAM = F(1.9e-4)                # rtk_walk.h kOwnLam
DIR_TOL = 2.0 ** -16               # rtk_math.h kPfDirTol


def fma(a, b, c):
    """RN_f32(a b + c) for f32 arrays, correctly rounded (v_fma_f32, fmaf).

    The product of two f32 is exact in f64 (48 bits, exponent in range).  s = RN_f64(p + c) and TwoSum's error term
    give the exact sum s + err; where it is inexact the f64 is rounded to odd instead (an even last bit steps one ulp
    towards the error), and a round-to-odd value of 53 bits rounds to 24 bits -- or to a subnormal's fewer -- as the
    exact sum does.  Infinities and NaN pass through the plain sum."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        step = np.isfinite(s) & (err != 0.0) & ((s.view(np.int64) & 1) == 0)
        odd = np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf))
        return np.where(step, odd, s).astype(F)


def bits(x):
    return np.ascontiguousarray(x, F).view(U)


def quiet(f):
    """f under numpy's errstate: NaN, infinities and overflow are inputs here, not accidents."""
    def run(*a, **k):
        with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
            return f(*a, **k)
    run.__name__, run.__doc__ = f.__name__, f.__doc__
    return run


@quiet
def dist_from_c(cx, cy, cz, dx, dy, dz):
    """(T, |C - D T|^2) from C = S - O: pair_dist_c, and the last 16 of pair_dist's 19 ops (main.cpp:402-407)."""
    T = (cx * dx + cy * dy) + cz * dz
    qx, qy, qz = cx - dx * T, cy - dy * T, cz - dz * T
    return T, (qx * qx + qy * qy) + qz * qz


@quiet
def sphere_core(o, d, s):
    """(T, dist) of sphere_core / pair_dist for origins o, directions d and centres s (last axis xyz, broadcast)."""
    o, d, s = (np.asarray(v, F) for v in (o, d, s))
    cx, cy, cz = (s[..., k] - o[..., k] for k in range(3))
    return dist_from_c(cx, cy, cz, d[..., 0], d[..., 1], d[..., 2])


@quiet
def candidate_it(T, dist, r2):
    """(it, inside) of candidate: X = sqrt(r2 - dist), it = T - X, or T + X where that is below eps."""
    X = np.sqrt((np.asarray(r2, F) - dist).astype(F))
    it = (T - X).astype(F)
    inside = it < EPS
    return np.where(inside, (T + X).astype(F), it).astype(F), inside


@quiet
def hit_test(simd, dist, r2, real=True):
    """The rule set's hit test: d < r^2 (main.cpp:409), or !(d > r^2) over the real spheres (main.cpp:547, 557)."""
    return (dist < r2) if simd else (~(dist > r2) & real)


class Hit:
    """rtk_walk.h Hit of n lanes: t (n, 4), k (n, 4), ins (n,)."""

    def __init__(self, n):
        self.t = np.full((n, 4), FMAX, F)
        self.k = np.zeros((n, 4), U)
        self.ins = np.zeros(n, U)

    def words(self):
        """The nine words a lane holds, as tests/walk_probe stores them."""
        return np.concatenate([bits(self.t), self.k, self.ins[:, None]], axis=1)


@quiet
def candidate(h, simd, g, L, T, dist, r2, called):
    """candidate<SIMD, L>(h, g, T, dist, r2) on the lanes of `called`."""
    it, inside = candidate_it(T, dist, r2)
    s = U(4 * g + L)
    if simd:
        acc = called & (it < h.t[:, L]) & (it > EPS)  # strict: the earliest group keeps a tie
        h.t[:, L] = np.where(acc, it, h.t[:, L])
        key = s | np.where(inside, KEY_INSIDE, U(0))
        h.k[:, L] = np.where(acc, (h.k[:, L] & KEY_INSIDE) | key, h.k[:, L])  # the class's flag is sticky
    else:
        acc = called & ~(it > h.t[:, 0]) & ~(it < EPS)  # the later sphere wins a tie
        h.t[:, 0] = np.where(acc, it, h.t[:, 0])
        h.k[:, 0] = np.where(acc, s, h.k[:, 0])
        h.ins = np.where(acc, inside.astype(U), h.ins)  # not sticky


def candidate_steps(simd, steps, gids):
    """tests/walk_probe's candidate entry: steps (S, n, 3) of {T, dist, r2}, step s to class s & 3 of group
    gids[s >> 2], called where the rule set's hit test passes."""
    S, n, _ = steps.shape
    h = Hit(n)
    for s in range(S):
        T, dist, r2 = steps[s, :, 0], steps[s, :, 1], steps[s, :, 2]
        candidate(h, simd, int(gids[s >> 2]), s & 3, T, dist, r2, hit_test(simd, dist, r2))
    return h


def group_rows(groups):
    """(centres (4 G, 3), r2 (4 G,), r2p (4 G,)) per sphere slot of packed group records (G, 5, 4)."""
    g = np.asarray(groups, F)
    return np.stack([g[:, 0].ravel(), g[:, 1].ravel(), g[:, 2].ravel()], 1), g[:, 3].ravel(), g[:, 4].ravel()


def group_walk(simd, o, d, groups, n_spheres, halves=(True, True), flags=None, c_rows=None):
    """test_group over the groups in order (halves: recheck_pairs' uniform f01, f23; flags (n, G): per-lane
    f01 | f23 << 1 of test_group_pf; c_rows (4 G, 3): the common origin's C = RN(S - O), test_pair_prim)."""
    centres, r2, _ = group_rows(groups)
    h = Hit(len(o))
    for s in range(len(r2)):
        g, L = divmod(s, 4)
        if not halves[L >> 1]:
            continue
        if c_rows is None:
            T, dist = sphere_core(o, d, centres[s][None, :])
        else:
            T, dist = dist_from_c(c_rows[s, 0], c_rows[s, 1], c_rows[s, 2], d[:, 0], d[:, 1], d[:, 2])
        called = hit_test(simd, dist, r2[s], s < n_spheres)
        if flags is not None:
            called = called & ((flags[:, g] >> (L >> 1)) & 1).astype(bool)
        candidate(h, simd, g, L, T, dist, np.broadcast_to(r2[s], T.shape), called)
    return h


@quiet
def prefilter(o, d, s):
    """(e, T, cc) of pair_prefilter: C = RN(S - O), cc = |C|^2 and T = C.D fused, e = fma(-T, T, cc)."""
    o, d, s = (np.asarray(v, F) for v in (o, d, s))
    cx, cy, cz = (s[..., k] - o[..., k] for k in range(3))
    cc = fma(cx, cx, fma(cy, cy, cz * cz))
    T = fma(cz, d[..., 2], fma(cy, d[..., 1], cx * d[..., 0]))
    return fma(-T, T, cc), T, cc


@quiet
def prefilter_flags(e, cc, r2p, rel):
    """prefilter_group's per-sphere flag !(e >= t), t = r2p or RN(cc kPfRel + r2p)."""
    t = fma(cc, PF_REL, r2p) if rel else np.broadcast_to(r2p, e.shape)
    return ~(e >= t)


def prefilter_group(o, d, groups, rel):
    """(n, G) words f01 | f23 << 1 of prefilter_group<REL>."""
    centres, _, r2p = group_rows(groups)
    e, _, cc = prefilter(o[:, None, :], d[:, None, :], centres[None, :, :])
    f = prefilter_flags(e, cc, r2p[None, :], rel).reshape(len(o), -1, 4)
    return ((f[:, :, 0] | f[:, :, 1]).astype(U) | ((f[:, :, 2] | f[:, :, 3]).astype(U) << U(1))).astype(U)


@quiet
def ray_expand(o, d, c0):
    """RayX of ray_expand, (n, 8): {-2O'x, Dx, -2O'y, Dy, -2O'z, Dz, |O'|^2, -O'.D}."""
    ox, oy, oz = ((o[:, k] - F(c0[k])).astype(F) for k in range(3))
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    oo = fma(ox, ox, fma(oy, oy, oz * oz))
    od = fma(ox, dx, fma(oy, dy, oz * dz))
    return np.stack([F(-2) * ox, dx, F(-2) * oy, dy, F(-2) * oz, dz, oo, -od], 1).astype(F)


@quiet
def prefilter_x(rx, s):
    """(e', T) of pair_prefilter_x for RayX rows rx (n, 8) against recentred centres s (m, 3): (n, m) each."""
    c = [rx[:, k][:, None] for k in range(8)]
    sx, sy, sz = (s[None, :, k] for k in range(3))
    T = fma(sx, c[1], fma(sy, c[3], fma(sz, c[5], c[7])))
    A = fma(sx, c[0], fma(sy, c[2], fma(sz, c[4], c[6])))
    return fma(-T, T, A), T


@quiet
def member_thr(cc, r):
    return fma(cc, PF_REL, r)


@quiet
def cluster_thr(cc, r, beta):
    """(t, b) = (RN(cc kClRel + R), RN(beta - cc kBehindRel))"""
    return fma(cc, CL_REL, r), fma(cc, -BEHIND_REL, beta)


@quiet
def cluster_slab(cc, T, oy, dy, srho, ymid, yhalf):
    """(d, thr) of cluster_slab with ClConst as clustered_groups builds it: d = RN(RN(D.y T + O.y) - ymid),
    thr = RN(|D.y| srho + RN(yhalf + E)), E = RN(cc kSlabRel + RN(|O.y| 2^-21 + kSlabRel))."""
    e0 = fma(np.abs(oy), F(2.0 ** -21), SLAB_REL)
    E = fma(cc, SLAB_REL, e0)
    thr = fma(np.abs(dy), srho, (yhalf + E).astype(F))
    d = (fma(dy, T, oy) - ymid).astype(F)
    return d, thr


@quiet
def own_parts(o, d, sc):
    c = [(sc[:, k] - o[:, k]).astype(F) for k in range(3)]
    cc = fma(c[0], c[0], fma(c[1], c[1], c[2] * c[2]))
    T = fma(c[2], d[:, 2], fma(c[1], d[:, 1], c[0] * d[:, 0]))
    return cc, T, fma(cc, -OWN_CC, sc[:, 3])


@quiet
def own_rule(o, d, sc):
    """own_sphere's test: True where the lane leaves its own sphere out (sc (n, 4) = {S, rho})."""
    _, T, dd = own_parts(o, d, sc)
    return np.abs(dd) < (T * -OWN_LAM).astype(F)


def own_sphere(o, d, sc, slot):
    return np.where(own_rule(o, d, sc), np.asarray(slot, U), OWN_NONE).astype(U)


@quiet
def origin_near(o, d, sc):
    _, _, dd = own_parts(o, d, sc)
    return np.abs(dd) < (sc[:, 3] * F(2.0 ** -6)).astype(F)


def same_bits(got, want):
    """(equal, both NaN, differing) counts and the mask of differing elements: bit patterns, except that a NaN
    equals any NaN (x86 and the GPU differ in the sign and payload they produce)."""
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert g.shape == w.shape, (g.shape, w.shape)
    both_nan = np.isnan(g) & np.isnan(w)
    diff = (g.view(U) != w.view(U)) & ~both_nan
    return int((~diff & ~both_nan).sum()), int(both_nan.sum()), int(diff.sum()), diff


def assert_same_bits(got, want, what):
    eq, nan, bad, diff = same_bits(got, want)
    if bad:
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        g, w = np.asarray(got, F)[at], np.asarray(want, F)[at]
        raise AssertionError(f"{what}: {bad} differ, {eq} equal, {nan} NaN on both sides; first at {at}: "
                             f"got {g!r} ({int(bits(g).ravel()[0]):#010x}), want {w!r} ({int(bits(w).ravel()[0]):#010x})")
    return eq, nan
