"""The walk layer of csrc/rtk_walk.h alone on the GPU, function by function, against tests/walk_ref.py.

tests/walk_probe runs the header's own pair tests (sphere_core, pair_dist, pair_dist_c), candidate logic, group tests
(test_group, recheck_pairs, test_group_pf, test_pair_prim), prefilters (pair_prefilter, prefilter_group, ray_expand,
pair_prefilter_x), per-lane thresholds (member_thr, cluster_thr, cluster_slab) and origin rules (own_sphere,
origin_near) one ray per lane, with the sphere operands in SGPRs as the walks hold them.  Every comparison is of bit
patterns, except that a NaN equals any NaN (walk_ref.same_bits; the counts of both-NaN elements are in every failure
message).  Rays have arbitrary origins on scene spheres, which rt_first_hit.hip's camera rays never give these
functions, half of them aimed at a silhouette, some lanes outside the |D|^2 bound of the prefilter, and a few with
0, -0, denormal and NaN components.  Every case runs 1,000 lanes (fifteen whole waves and one of 40) in both tail
forms: lanes past the count computing on a clamped index, and lanes past the count gone (partial exec).

Besides equality with the restatement, the prefilter cases check the skip proofs' condition on the DEVICE's own
numbers, with no allowance: no pair that holds a sphere the reference-rounded exact test can accept
(test_prefilter_bound.could_accept) has a clear flag.  The CPU proofs (test_prefilter_bound, test_expanded_prefilter,
test_own_sphere_skip) assert the same of the restatement, which the cases here show to be the device's arithmetic.

What this file cannot see: the table walks (clustered_groups, member_pairs, cluster_pair, direction_*, wave_or: they
stay with their frame tests), the hit select spelled inline in the trace kernels, register pressure and cost.
"""
import functools

import numpy as np
import pytest

import test_expanded_prefilter as txp
import test_own_sphere_skip as town
import test_prefilter_bound as tpb
import walk_probe as wp
import walk_ref as wr
from test_walk_ref import GIDS, crafted_steps, random_steps

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
N = 1000  # fifteen whole waves and one of 40 lanes; four blocks, the last one short
SCENES = [(1, 64), (1, 256), (0, None), (2, None)]  # test_prefilter_never_skips_an_exact_hit's
EARLY = [0, 1]


@pytest.fixture(scope="module")
def gpu(torch_cuda):
    wp.lib()
    return torch_cuda


def edge_rays(o, d):
    """The rays with a few lanes of every wave replaced: zero, -0 and denormal components, a NaN component, a zero
    direction, and lanes outside the prefilter's |D|^2 bound.  Returns (o, d, lanes that are finite and inside it)."""
    o, d = o.copy(), d.copy()
    for base in range(0, len(o) - 24, 64):
        o[base + 3, 0] = 0.0
        o[base + 4, 1] = -0.0
        o[base + 5, 2], d[base + 5, 0] = F(1e-40), F(-3e-41)
        d[base + 6, 1] = np.nan
        o[base + 7, 0] = np.nan
        d[base + 8] = 0.0
        d[base + 9] = (d[base + 9] * F(1.01)).astype(F)
        d[base + 10] = (d[base + 10] * F(0.5)).astype(F)
        o[base + 11], d[base + 11, 2] = 0.0, -0.0
    fin = np.isfinite(o).all(1) & np.isfinite(d).all(1)
    with np.errstate(invalid="ignore"):
        inside = fin & (np.abs(1.0 - (d.astype(np.float64) ** 2).sum(1)) <= wr.DIR_TOL)
    return o, d, inside


class Case:
    def __init__(self, rt, idx, n_spheres, simd):
        scene = rt.scene_builtin(idx)
        if n_spheres:
            scene = rt.scene_prefix(scene, n_spheres)
        self.rt, self.scene, self.simd = rt, scene, simd
        self.r2, self.r2p, self.flags = rt.scene_prefilter(scene, simd)
        self.fast, self.rel = bool(self.flags & 2), bool(self.flags & 4)
        self.groups = rt.scene_groups(scene, simd)[0]
        self.n_spheres = scene.ScalarSpheres.Count
        self.centres, radius = tpb.slot_spheres(rt, scene, simd)
        c, r2, r2p = wr.group_rows(self.groups)
        assert np.array_equal(c, self.centres) and np.array_equal(wr.bits(r2), wr.bits(self.r2))
        assert np.array_equal(wr.bits(r2p), wr.bits(self.r2p)), "the packed records are what rt_scene_prefilter reports"
        self.live = self.r2 > 0 if simd else self.r2 >= 0
        rng = np.random.default_rng(1000 + 10 * idx + (n_spheres or 0) + int(simd))
        o, d = tpb.rays(rng, self.centres[self.live], np.abs(radius[self.live]).astype(F), N)
        self.o, self.d, self.inside = edge_rays(o, d)
        assert 0.85 * N < self.inside.sum() < N


@functools.lru_cache(maxsize=None)
def _case(rt, idx, n_spheres, simd):
    return Case(rt, idx, n_spheres, simd)


@pytest.fixture(params=[(i, n, s) for i, n in SCENES for s in (True, False)],
                ids=lambda p: f"scene{p[0]}-{p[1] or 'all'}-{'simd' if p[2] else 'scalar'}")
def case(request, rt, gpu):
    return _case(rt, *request.param)


def same(got, want, what):
    return wr.assert_same_bits(got, want, what)


def same_hit(got, want, what):
    """Hit words (n, 9): the four t as floats (NaN equals NaN), the keys and `ins` as integers."""
    same(got[:, :4].view(F), want[:, :4].view(F), what + ": t")
    bad = np.argwhere(got[:, 4:] != want[:, 4:])
    assert len(bad) == 0, (f"{what}: {len(bad)} key / ins words differ; first at lane {bad[0][0]} word {4 + bad[0][1]}: "
                           f"got {got[bad[0][0], 4 + bad[0][1]]:#x}, want {want[bad[0][0], 4 + bad[0][1]]:#x}")


# ---- exact: sphere_core, pair_dist, pair_dist_c

@pytest.mark.parametrize("early", EARLY)
def test_exact_pair_tests(case, early):
    c = case
    T, dist = wr.sphere_core(c.o[:, None, :], c.d[:, None, :], c.centres[None, :, :])
    Tc, dc = wp.exact(c.o, c.d, c.centres, "core", early)
    Tp, dp = wp.exact(c.o, c.d, c.centres, "pair", early)
    _, nan = same(dc, dist, "sphere_core dist")
    same(Tc, T, "sphere_core T"), same(Tp, T, "pair_dist T"), same(dp, dist, "pair_dist dist")
    same(Tp, Tc, "pair_dist T against sphere_core's"), same(dp, dc, "pair_dist dist against sphere_core's")
    assert nan >= 2 * (N // 64) * len(c.centres), "the NaN rays are among the lanes"
    # one common origin (a point on a sphere, not a camera): the rows C = RN(S - O) as prim_kernel forms them
    o0 = np.broadcast_to(c.o[1], c.o.shape).copy()
    rows = (c.centres - c.o[1][None, :]).astype(F)
    T0, d0 = wr.dist_from_c(rows[None, :, 0], rows[None, :, 1], rows[None, :, 2], c.d[:, 0:1], c.d[:, 1:2], c.d[:, 2:3])
    Tq, dq = wp.exact(o0, c.d, rows, "c", early)
    Tr, dr = wp.exact(o0, c.d, c.centres, "pair", early)
    same(Tq, T0, "pair_dist_c T"), same(dq, d0, "pair_dist_c dist")
    same(Tq, Tr, "pair_dist_c T against pair_dist's"), same(dq, dr, "pair_dist_c dist against pair_dist's")


# ---- candidate

@pytest.mark.parametrize("early", EARLY)
@pytest.mark.parametrize("simd", [True, False], ids=["simd", "scalar"])
def test_candidate_sequences(gpu, simd, early):
    crafted, _ = crafted_steps(N)
    rnd = random_steps(np.random.default_rng(21 + int(simd)), N, 4 * len(GIDS))
    for name, steps in (("crafted", crafted), ("random", rnd)):
        want = wr.candidate_steps(simd, steps, GIDS).words()
        slow = wp.candidate(steps, GIDS, simd, 0, early)
        fast = wp.candidate(steps, GIDS, simd, 1, early)
        same_hit(slow, want, f"{name}, IEEE sqrt")
        same_hit(fast, want, f"{name}, sqrt_rn")  # every r2 - dist here is 0, NaN or inside [2^-60, 2^60]
        assert (want[:, 4:8] >> 31).any() or not simd
        assert np.isnan(want[:, 0].view(F)).any() != simd, "scalar rules alone accept a NaN dist"


# ---- group: test_group, recheck_pairs, test_group_pf, test_pair_prim

@pytest.mark.parametrize("early", EARLY)
def test_group_tests_agree(case, early):
    c = case
    run = lambda variant, o=c.o, **k: wp.group(o, c.d, c.groups, c.n_spheres, variant, c.simd, c.fast, early, **k)
    want = wr.group_walk(c.simd, c.o, c.d, c.groups, c.n_spheres).words()
    full = run("test_group")
    same_hit(full, want, "test_group")
    same_hit(run("recheck11"), want, "recheck_pairs(1, 1)")
    hits = (want[:, :4].view(F) != wr.FMAX).any(1)
    assert hits.sum() > N // 20 and (~hits).sum() > N // 20, "rays that hit and rays that miss"
    for variant, halves in (("recheck00", (False, False)), ("recheck10", (True, False)), ("recheck01", (False, True))):
        w = wr.group_walk(c.simd, c.o, c.d, c.groups, c.n_spheres, halves=halves).words()
        same_hit(run(variant), w, variant)
    # the prefiltered test: the restatement's flags decide which pairs are rechecked; inside the |D|^2 bound the
    # skipped pairs are proven misses, so the Hit is test_group's
    flags = wr.prefilter_group(c.o, c.d, c.groups, c.rel)
    pf = run("pf", rel=c.rel)
    same_hit(pf, wr.group_walk(c.simd, c.o, c.d, c.groups, c.n_spheres, flags=flags).words(), "test_group_pf")
    same_hit(pf[c.inside], full[c.inside], "test_group_pf against test_group inside the |D|^2 bound")
    skipped = ((flags & 1) == 0).sum() + ((flags & 2) == 0).sum()
    assert skipped > flags.size // 2, "the prefilter skips pairs on these rays"
    # one common origin: every pair in ascending order through test_pair_prim
    o0 = np.broadcast_to(c.o[1], c.o.shape).copy()
    rows = (c.centres - c.o[1][None, :]).astype(F)
    prim = np.stack([rows[:, 0].reshape(-1, 4), rows[:, 1].reshape(-1, 4), rows[:, 2].reshape(-1, 4),
                     c.r2.reshape(-1, 4)], axis=1)
    w0 = wr.group_walk(c.simd, o0, c.d, c.groups, c.n_spheres, c_rows=rows).words()
    got = run("prim", o=o0, prim=prim)
    same_hit(got, w0, "test_pair_prim")
    same_hit(got, run("test_group", o=o0), "test_pair_prim against test_group")


@pytest.mark.parametrize("n_spheres", [13, 14, 15])
def test_ragged_last_group_and_a_point_sphere_under_the_scalar_rules(rt, gpu, n_spheres):
    """n_spheres % 4 of 1, 2 and 3: the padding slots (centre 0, r^2 = -inf) are never candidates, also for rays
    through the origin; sphere 2 has r = 0, which the scalar rules can hit (!(d > 0) at d = 0) and the SIMD rules
    cannot."""
    sp = rt.scene_arrays(rt.scene_prefix(rt.scene_builtin(1), n_spheres))[0].copy()
    sp[2, 4] = 0.0
    scene = rt.scene_from_spheres(sp)
    for simd in (False, True):
        groups = rt.scene_groups(scene, simd)[0]
        r2, _, flags = rt.scene_prefilter(scene, simd)
        if not simd:
            assert np.all(np.isneginf(r2[n_spheres:])) and r2[2] == 0.0 and len(r2) == 16
        centres, radius = tpb.slot_spheres(rt, scene, simd)
        rng = np.random.default_rng(n_spheres)
        o, d = tpb.rays(rng, centres[:n_spheres], np.maximum(np.abs(radius[:n_spheres]), F(0.05)).astype(F), N)
        o, d, _ = edge_rays(o, d)
        # rays through the padding's centre (the origin) and through the point sphere's centre, exactly
        for k, target in ((20, np.zeros(3, F)), (21, centres[2])):
            d[k::64] = (target[None, :] - o[k::64]).astype(F)
        o[22::64], d[22::64] = centres[2], np.array([0.0, 0.0, 1.0], F)  # starts on the point itself: d = 0, it = 0
        o[23::64], d[23::64] = (centres[2] - np.array([0, 0, 2], F)).astype(F), np.array([0.0, 0.0, 1.0], F)
        want = wr.group_walk(simd, o, d, groups, n_spheres).words()
        if not simd:
            assert not np.isin(want[:, 4], np.arange(n_spheres, 16)).any(), "a padding slot was hit"
            assert (want[23::64, 4] == 2).all() and (want[23::64, 0].view(F) == F(2.0)).all(), "the point sphere is hit"
        else:
            assert not (want[23::64, 4:8] == 2).any()
        for early in EARLY:
            for variant in ("test_group", "recheck11"):
                got = wp.group(o, d, groups, n_spheres, variant, simd, bool(flags & 2), early)
                same_hit(got, want, f"{variant}, simd={simd}, early={early}")


# ---- prefilter: pair_prefilter, prefilter_group

@pytest.mark.parametrize("early", EARLY)
def test_prefilter_is_the_restatement_and_never_skips_an_exact_hit(case, early):
    c = case
    e, T, cc = wp.prefilter(c.o, c.d, c.centres, early)
    we, wT, wcc = wr.prefilter(c.o[:, None, :], c.d[:, None, :], c.centres[None, :, :])
    same(e, we, "e"), same(T, wT, "T"), same(cc, wcc, "cc")  # (a), rays outside the |D|^2 bound among them
    cx, cy, cz = (c.centres[None, :, k] - c.o[:, None, k] for k in range(3))
    dx, dy, dz = c.d[:, None, 0], c.d[:, None, 1], c.d[:, None, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        pe, pT, pcc = tpb.prefilter(cx, cy, cz, np.broadcast_to(dx, cx.shape), np.broadcast_to(dy, cx.shape),
                                    np.broadcast_to(dz, cx.shape), with_cc=True)
    same(e, pe, "e against the CPU proof's"), same(T, pT, "T against the CPU proof's"), same(cc, pcc, "cc, likewise")
    for rel in (c.rel, not c.rel):
        got = wp.prefilter_group(c.o, c.d, c.groups, rel, early)
        assert np.array_equal(got, wr.prefilter_group(c.o, c.d, c.groups, rel)), f"prefilter_group<{rel}> flags"
    # (b) on the device's own e and cc, by the proof's own threshold function, and on the device's own flags
    flags = wp.prefilter_group(c.o, c.d, c.groups, c.rel, early)
    with np.errstate(invalid="ignore", over="ignore"):
        accept = tpb.could_accept(cx, cy, cz, dx, dy, dz, c.r2[None, :], c.simd) & c.live[None, :]
        skipped = ~(e < tpb.threshold(c.r2p[None, :], cc, c.rel))
    accept, skipped = accept[c.inside], skipped[c.inside]
    pair_flag = np.repeat(((flags[:, :, None] >> np.arange(2, dtype=U)[None, None, :]) & 1).reshape(N, -1), 2, axis=1) != 0
    pair_flag = pair_flag[c.inside]
    assert pair_flag.shape == accept.shape
    print(f"accepted {int(accept.sum())}, skipped spheres {int((skipped & c.live[None, :]).sum())}, "
          f"clear pair flags {int((~pair_flag).sum())} of {pair_flag.size}")
    assert accept.sum() > 0 and (skipped & c.live[None, :]).sum() > 0 and (~pair_flag).sum() > 0, "vacuous inputs"
    assert not np.any(accept & skipped), "the device's e is at its threshold on a sphere the exact test accepts"
    assert not np.any(accept & ~pair_flag), "a pair with a clear flag holds a sphere the exact test accepts"
    assert not np.any(~skipped & ~pair_flag), "a flag is clear although the device's own e is below the threshold"


# ---- expanded: ray_expand, pair_prefilter_x

@pytest.mark.parametrize("early", EARLY)
def test_expanded_prefilter_is_the_restatement_and_never_skips_an_exact_hit(rt, gpu, early):
    ran = 0
    for idx, n_spheres in SCENES:
        for simd in (True, False):
            c = _case(rt, idx, n_spheres, simd)
            if rt.scene_clusters_expanded(c.scene, simd)[0].shape[0] == 0:
                continue  # no scene-wide table (none at all, or per-lane thresholds)
            ran += 1
            tab, xtab, c0, use, clusters, member_of = txp.decode(rt, c.scene, simd)
            assert use
            rx = wp.expand(c.o, c.d, c0, early)
            same(rx, wr.ray_expand(c.o, c.d, c0), "RayX")
            # every entry of the table, cluster pairs and member pairs alike: both halves are one sphere pair
            sp = np.stack([xtab[:, 0, 0:2], xtab[:, 0, 2:4], xtab[:, 1, 0:2]], axis=2).reshape(-1, 3)
            e, T = wp.prefilter_x(c.o, c.d, c0, sp, early)
            we, wT = wr.prefilter_x(wr.ray_expand(c.o, c.d, c0), sp)
            same(e, we, "e'"), same(T, wT, "T of the expanded form")
            slots = np.array(sorted(member_of))
            ent = np.array([member_of[s][0] for s in slots])
            half = np.array([member_of[s][1] for s in slots])
            with np.errstate(invalid="ignore", over="ignore"):
                pnear, pbehind, pT = txp.expanded(xtab, c0, c.o, c.d, ent, half)
                near = e[:, 2 * ent + half] >= xtab[ent, 1, 2 + half][None, :]
                behind = T[:, 2 * ent + half] < xtab[ent, 3, half][None, :]
            same(T[:, 2 * ent + half], pT, "T against the CPU proof's")
            assert np.array_equal(near, pnear) and np.array_equal(behind, pbehind)
            # (b) on the device's own e' and T
            cx, cy, cz = (c.centres[None, :, k] - c.o[:, None, k] for k in range(3))
            with np.errstate(invalid="ignore", over="ignore"):
                accept = tpb.could_accept(cx, cy, cz, c.d[:, None, 0], c.d[:, None, 1], c.d[:, None, 2], c.r2[None, :],
                                          simd) & np.isfinite(c.r2p)[None, :]
            accept, near, behind = accept[c.inside][:, slots], near[c.inside], behind[c.inside]
            print(f"accepted {int(accept.sum())}, near-line skips {int(near.sum())}, behind skips {int(behind.sum())}")
            assert accept.sum() > 0 and near.sum() > 0 and behind.sum() > 0, "vacuous inputs"
            assert not np.any(accept & near), "e' >= t' on a sphere the exact test accepts"
            assert not np.any(accept & behind), "T < b' on a sphere the exact test accepts"
            for en, h, ms in clusters:
                if np.isneginf(xtab[en, 1, 2 + h]) or not ms:
                    continue
                with np.errstate(invalid="ignore"):
                    skip = (e[:, 2 * en + h] >= xtab[en, 1, 2 + h]) | (T[:, 2 * en + h] < xtab[en, 3, h])
                cols = np.searchsorted(slots, np.array(ms))
                assert not np.any(accept[skip[c.inside]][:, cols]), "a skipped cluster holds a sphere a lane can accept"
    assert ran == 4, "Floating Spheres at 64 and 256 spheres, both rule sets, have the expanded table"


# ---- thresholds: member_thr, cluster_thr, cluster_slab

@pytest.mark.parametrize("early", EARLY)
@pytest.mark.parametrize("simd", [True, False], ids=["simd", "scalar"])
def test_per_lane_thresholds(rt, gpu, simd, early):
    """On RTWeekend's per-lane table: every cluster-pair entry's R, beta, srho, ymid and yhalf rows, with cc and T of
    the lane's ray against the entry-0 pair (and a few lanes of 0, denormal, huge, infinite and NaN cc)."""
    c = _case(rt, 2, None, simd)
    assert c.rel
    tab, ncp = rt.scene_clusters(c.scene, simd)
    levels, n_sub = rt.scene_cluster_layout(c.scene, simd)
    n_cl = ncp + (n_sub if levels == 2 else 0)
    assert tab.shape[1] >= 5 and n_cl >= 8
    q = tab[:n_cl]
    entries = np.zeros((n_cl, 3, 4), F)
    entries[:, 0, 0:2], entries[:, 0, 2:4] = q[:, 1, 2:4], q[:, 3, 0:2]
    entries[:, 1, 0:2], entries[:, 1, 2:4] = q[:, 3, 2:4], q[:, 4, 0:2]
    entries[:, 2, 0:2] = q[:, 4, 2:4]
    pair0 = np.stack([q[0, 0, 0:2], q[0, 0, 2:4], q[0, 1, 0:2]], axis=1)
    _, T, cc = wr.prefilter(c.o[:, None, :], c.d[:, None, :], pair0[None, :, :])
    T, cc = T.copy(), cc.copy()
    for base in range(0, N - 24, 64):
        cc[base + 12], cc[base + 13], cc[base + 14] = 0.0, F(1e-41), F(3e38)
        cc[base + 15], cc[base + 16], T[base + 17] = np.inf, np.nan, np.nan
    got = wp.thresholds(c.o, c.d, cc, T, entries, early)
    R, beta = entries[None, :, 0, 0:2], entries[None, :, 0, 2:4]
    srho, ymid, yhalf = entries[None, :, 1, 0:2], entries[None, :, 1, 2:4], entries[None, :, 2, 0:2]
    ccb, Tb = np.broadcast_to(cc[:, None, :], got["member_t"].shape), np.broadcast_to(T[:, None, :], got["member_t"].shape)
    oy, dy = (np.broadcast_to(v[:, None, None], ccb.shape) for v in (c.o[:, 1], c.d[:, 1]))
    same(got["member_t"], wr.member_thr(ccb, R), "member_thr")
    wt, wb = wr.cluster_thr(ccb, R, beta)
    same(got["cluster_t"], wt, "cluster_thr t"), same(got["cluster_b"], wb, "cluster_thr b")
    wd, wthr = wr.cluster_slab(ccb, Tb, oy, dy, srho, ymid, yhalf)
    same(got["slab_d"], wd, "cluster_slab d"), same(got["slab_thr"], wthr, "cluster_slab thr")
    # ... and the CPU proof's own spellings (test_prefilter_bound), on the device's numbers for the slab's two sides
    Rb, betab = np.broadcast_to(R, ccb.shape), np.broadcast_to(beta, ccb.shape)
    same(got["member_t"], tpb.threshold(Rb, ccb, True), "member_thr against threshold()")
    same(got["cluster_t"], tpb.cluster_threshold(Rb, ccb, True), "cluster_thr against cluster_threshold()")
    same(got["cluster_b"], tpb.behind_threshold(betab, ccb, True), "cluster_thr against behind_threshold()")
    skips = 0
    for en in range(n_cl):
        for h in range(2):
            with np.errstate(invalid="ignore"):
                dev = np.abs(got["slab_d"][:, en, h]) > got["slab_thr"][:, en, h]
            ref = tpb.slab_skip(T[:, h], cc[:, h], c.o[:, 1], c.d[:, 1], entries[en, 1, h], entries[en, 1, 2 + h],
                                entries[en, 2, h])
            assert np.array_equal(dev, ref), f"slab_skip, entry {en} half {h}"
            skips += int(dev.sum())
    assert 0 < skips < 2 * n_cl * N, "the slab rule skips some and not all"


# ---- own_sphere, origin_near

def own_inputs(rt, scene, simd, seed):
    """test_own_sphere_skip's landings and new directions on a scene: (o, d, sphere slot) of N lanes, all four kinds of
    direction, a quarter of the origins pushed off the surface."""
    r2 = rt.scene_prefilter(scene, simd)[0]
    centres, radius = tpb.slot_spheres(rt, scene, simd)
    radius = np.abs(radius).astype(F)
    live = np.flatnonzero((r2 > 0 if simd else r2 >= 0) & np.isfinite(r2) & (radius > 0))
    rng = np.random.default_rng(seed)
    os_, ds_, js_ = [], [], []
    for src in town.camera_positions(rt, scene) + [None]:
        n = 400
        j = rng.choice(live, n)
        if src is None:
            i = rng.choice(live, n)
            prev_o = centres[i].astype(np.float64) + radius[i, None] * tpb.unit(rng.normal(size=(n, 3)))
        else:
            prev_o = np.broadcast_to(src, (n, 3)).copy()
        o, dprev, jj, _ = town.landings(rng, centres, radius, r2, j, prev_o)
        off = np.where(rng.random((len(o), 1)) < 0.25, 10.0 ** rng.uniform(-8, -2, (len(o), 1)), 0.0)
        off *= rng.choice([-1.0, 1.0], (len(o), 1))
        o = (o + ((o - centres[jj]) * off).astype(F)).astype(F)
        for d in town.new_directions(rng, o, dprev, centres, jj).values():
            os_.append(o), ds_.append(d), js_.append(jj)
    o, d, j = np.concatenate(os_), np.concatenate(ds_), np.concatenate(js_)
    pick = rng.permutation(len(o))[:N]
    assert len(pick) == N
    return o[pick], d[pick], j[pick].astype(U), centres


@pytest.mark.parametrize("early", EARLY)
@pytest.mark.parametrize("simd", [True, False], ids=["simd", "scalar"])
@pytest.mark.parametrize("n_spheres", [64, 256])
def test_own_sphere_and_origin_near(rt, gpu, n_spheres, simd, early):
    scene = rt.scene_prefix(rt.scene_builtin(1), n_spheres)
    o, d, j, centres = own_inputs(rt, scene, simd, 300 + n_spheres + int(simd))
    rho = rt.scene_own_sphere(scene, simd)[j].astype(F)
    assert np.all(np.isfinite(rho)), "C2: the rule is on for every sphere"
    rho[5::64], rho[6::64] = np.inf, np.nan  # nothing is proven for these lanes
    sc = np.concatenate([centres[j], rho[:, None]], axis=1).astype(F)
    own, near = wp.own(o, d, sc, j, early)
    assert np.array_equal(own, wr.own_sphere(o, d, sc, j)), "own_sphere"
    assert np.array_equal(near, wr.origin_near(o, d, sc)), "origin_near"
    cx, cy, cz = (sc[:, k] - o[:, k] for k in range(3))
    proof = town.own_rule(cx, cy, cz, d[:, 0], d[:, 1], d[:, 2], rho)
    assert np.array_equal(own != wr.OWN_NONE, proof), "own_sphere against the CPU proof's own_rule"
    assert np.array_equal(own[own != wr.OWN_NONE], j[own != wr.OWN_NONE]), "a lane names the slot it was given"
    for k in (5, 6):
        assert np.all(own[k::64] == wr.OWN_NONE) and not near[k::64].any(), "rho = +inf or NaN: nothing"
    fired = int((own != wr.OWN_NONE).sum())
    assert N // 10 < fired < N - N // 10 and N // 2 < near.sum() < N, (fired, int(near.sum()))
