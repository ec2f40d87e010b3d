"""CPU tests of tests/walk_ref.py, the numpy restatements that tests/test_gpu_walk_layer.py holds the device's walk
layer to, and that the three CPU skip proofs (test_prefilter_bound, test_expanded_prefilter, test_own_sphere_skip)
run on.  Each restatement is compared with something that is not it: the fma with rational arithmetic, dist and the
candidate's t with the oracle's own SSE group test, the vectorised Hit update with a plain per-lane loop written from
the reference's text, and the own-sphere rule and thresholds with the proofs' own spellings."""
from fractions import Fraction

import numpy as np
import pytest

import test_own_sphere_skip
import test_prefilter_bound as tpb
import walk_ref as wr

F, U = np.float32, np.uint32


def rn_f32(q: Fraction) -> float:
    """q rounded to the nearest f32, ties to even, subnormals and overflow included (q != 0)."""
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    ulp = Fraction(2) ** (max(e, -126) - 23)
    r = round(q / ulp) * ulp  # (Fraction's round: half to even)
    if abs(r) >= Fraction(2) ** 128:
        r = np.inf
    return float(np.copysign(float(abs(r)), 1.0 if q > 0 else -1.0))  # (a result that rounds to zero keeps q's sign)


def f32_of(rng, n, emin, emax):
    """n f32 with random sign, full random mantissa and an exponent uniform in [emin, emax]."""
    m = rng.integers(0, 1 << 23, n).astype(U)
    e = rng.integers(emin + 127, emax + 128, n).astype(U)
    s = rng.integers(0, 2, n).astype(U)
    return ((s << U(31)) | (e << U(23)) | m).view(F)


def check_against_fractions(a, b, c):
    """wr.fma(a, b, c) against rational arithmetic, element by element; returns the plain f64 form's miss count."""
    got = wr.fma(a, b, c)
    with np.errstate(over="ignore"):
        plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    plain_wrong = 0
    for k in range(len(a)):
        q = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        if q == 0:  # (the sign of an exact zero: both forms take it from the same f64 sum)
            assert got[k] == 0.0
            continue
        want = F(rn_f32(q))
        assert got[k].view(U) == want.view(U), (a[k], b[k], c[k], got[k], want)
        plain_wrong += int(plain[k].view(U) != want.view(U))
    return plain_wrong


def test_exact_fma_on_random_triples():
    """10^5 triples: normal range at large, sums that cancel to a few bits, and addends far above or below the product."""
    rng = np.random.default_rng(1)
    n = 25_000
    a = np.concatenate([f32_of(rng, n, -30, 30) for _ in range(4)])
    b = np.concatenate([f32_of(rng, n, -30, 30) for _ in range(4)])
    c = f32_of(rng, 4 * n, -60, 60)
    with np.errstate(over="ignore"):
        p = (a * b).astype(F)
    c[n:2 * n] = -p[n:2 * n]                                         # cancels to the product's own rounding error
    c[2 * n:3 * n] = (-p[2 * n:3 * n] * F(1.0 + 2.0 ** -20)).astype(F)  # cancels to about 20 bits below
    c[3 * n:] = (p[3 * n:] * f32_of(rng, n, -26, 26)).astype(F)       # the addend within 2^26 either way of the product
    assert len(a) >= 100_000
    check_against_fractions(a, b, c)


def double_rounding_family(rng, n):
    """Triples whose exact sum lies within a quarter of an f64 ulp of an f32 midpoint, on the side RN-even leaves:
    a = 1 + x 2^-23, b = +-2^-24 (1 - x 2^-23) (x < 362: a b = +-2^-24 (1 - x^2 2^-46)), c an f32 of [1, 2) or just
    below 1, all scaled by powers of two.  The f64 sum is the midpoint itself, which then rounds to even."""
    x = rng.integers(1, 362, n).astype(np.float64)
    k = rng.integers(0, 1 << 23, n).astype(np.float64)
    down = rng.random(n) < 0.5
    a = (1.0 + x * 2.0 ** -23)
    b = np.where(down, -(2.0 ** -25), 2.0 ** -24) * (1.0 - x * 2.0 ** -23)
    c = np.where(down, 1.0 - (k % 4096 + 1) * 2.0 ** -24, 1.0 + k * 2.0 ** -23)
    ea, ec = rng.integers(-20, 21, n), rng.integers(-20, 21, n)
    sign = rng.choice([-1.0, 1.0], n)
    a, b, c = a * 2.0 ** ea, sign * b * 2.0 ** (ec - ea), sign * c * 2.0 ** ec
    out = tuple(v.astype(F) for v in (a, b, c))
    assert all(np.array_equal(v.astype(np.float64), w) for v, w in zip(out, (a, b, c))), "the family is exact in f32"
    return out


def test_exact_fma_where_the_plain_f64_form_double_rounds():
    """Found by search over the family above and over random triples: the triples on which the plain form
    (a64 b64 + c64 rounded to f32) and the exact one disagree.  Rational arithmetic sides with the exact one on
    every one of them, so the plain form is wrong there."""
    rng = np.random.default_rng(2)
    a, b, c = double_rounding_family(rng, 200_000)
    ra, rb = f32_of(rng, 2_000_000, -4, 4), f32_of(rng, 2_000_000, -4, 4)
    rc = f32_of(rng, 2_000_000, -4, 4)
    a, b, c = np.concatenate([a, ra]), np.concatenate([b, rb]), np.concatenate([c, rc])
    plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    found = np.flatnonzero(plain.view(U) != wr.fma(a, b, c).view(U))
    assert len(found) >= 10_000, len(found)
    pick = found[:: max(1, len(found) // 20_000)][:20_000]
    wrong = check_against_fractions(a[pick], b[pick], c[pick])
    assert wrong == len(pick)
    print(f"plain f64 fma wrong on {len(found)} of {len(a)} searched triples; {len(pick)} of them checked exactly")


def test_exact_fma_on_subnormal_results():
    """Results below 2^-126, and those that round up to it: products of about 2^-135 .. 2^-120 with subnormal, tiny
    normal, cancelling and zero addends."""
    rng = np.random.default_rng(3)
    n = 5_000
    a = np.concatenate([f32_of(rng, n, -70, -60) for _ in range(4)])
    b = np.concatenate([f32_of(rng, n, -75, -60) for _ in range(4)])
    sub = (rng.integers(0, 1 << 23, n).astype(U) | (rng.integers(0, 2, n).astype(U) << U(31))).view(F)
    tiny = f32_of(rng, n, -126, -120)
    p = (a * b).astype(F)
    c = np.concatenate([sub, tiny, -p[2 * n:3 * n], np.zeros(n, F)])
    want_sub = np.abs(wr.fma(a, b, c)) < F(2.0 ** -126)
    assert want_sub.sum() > 6_000 and (~want_sub).sum() > 1_000, (int(want_sub.sum()), len(a))
    check_against_fractions(a, b, c)
    # the smallest subnormal's neighbourhood: halves of it, from either side
    a2 = np.array([2.0 ** -75, 2.0 ** -75, 2.0 ** -75 * (1 + 2.0 ** -23), -(2.0 ** -75), 2.0 ** -63 * 1.5], F)
    b2 = np.array([2.0 ** -75, 2.0 ** -75, 2.0 ** -75, 2.0 ** -75, 2.0 ** -63 * (1 - 2.0 ** -24)], F)
    c2 = np.array([0.0, 2.0 ** -149, 0.0, 2.0 ** -149, 2.0 ** -149], F)
    check_against_fractions(a2, b2, c2)


def test_exact_fma_passes_infinities_and_nan_through():
    inf, nan = F(np.inf), F(np.nan)
    a = np.array([inf, 1.0, inf, nan, 3e38, -3e38, 0.0], F)
    b = np.array([1.0, 1.0, 0.0, 1.0, 3e38, 3e38, inf], F)
    c = np.array([1.0, -inf, 1.0, 1.0, 0.0, 0.0, 1.0], F)
    got = wr.fma(a, b, c)
    assert got[0] == inf and got[1] == -inf and np.isnan(got[2]) and np.isnan(got[3])
    assert got[4] == inf and got[5] == -inf and np.isnan(got[6])


def test_dist_and_candidate_t_against_the_oracle(rt, orc):
    """sphere_core's dist and candidate's it against the oracle's SSE group test (or_group_test: main.cpp:400-417)
    on more than 10^4 (ray, group) pairs, half of the rays aimed at a silhouette; NaN compares as NaN."""
    scene = rt.scene_prefix(rt.scene_builtin(1), 256)
    centres, radius = tpb.slot_spheres(rt, scene, True)
    groups = rt.scene_arrays(scene)[1]  # (G, 16): x[4], y[4], z[4], r[4]
    o, d = tpb.rays(np.random.default_rng(5), centres, np.abs(radius).astype(F), 200)
    assert len(o) * len(groups) >= 10_000
    r2 = (radius * radius).astype(F)
    T, dist = wr.sphere_core(o[:, None, :], d[:, None, :], centres[None, :, :])
    it, _ = wr.candidate_it(T, dist, r2[None, :])
    L = orc.lib()
    want_d, want_t = np.zeros_like(dist), np.zeros_like(it)
    d4, t4 = np.zeros(4, F), np.zeros(4, F)
    for i in range(len(o)):
        oi, di = np.ascontiguousarray(o[i]), np.ascontiguousarray(d[i])
        for g in range(len(groups)):
            L.or_group_test(oi.ctypes.data, di.ctypes.data, groups[g].ctypes.data, d4.ctypes.data, t4.ctypes.data)
            want_d[i, 4 * g:4 * g + 4], want_t[i, 4 * g:4 * g + 4] = d4, t4
    # near-tangent: dist within the prefilter bound's own allowance for f32 rounding, 32 u |C|^2, of r^2
    cc = ((centres[None, :, :].astype(np.float64) - o[:, None, :]) ** 2).sum(-1)
    near = np.abs(dist.astype(np.float64) - r2[None, :]) <= 32 * 2.0 ** -24 * cc
    assert near.sum() >= 20, "no near-tangent pairs: too tame"
    wr.assert_same_bits(dist, want_d, "dist")
    eq, nan = wr.assert_same_bits(it, want_t, "it")
    assert nan > 0 and eq > nan // 100, "both misses (NaN root) and hits"


def plain_hit_loop(simd, steps, gids):
    """The reference's loop state per lane, written from main.cpp:413-429 (per-class strict <, sticky inside bit,
    the earliest group keeps a tie) and main.cpp:561-578 (one slot, a later sphere wins a tie, flag not sticky)."""
    S, n, _ = steps.shape
    out = np.zeros((n, 9), U)
    eps = float(wr.EPS)
    for i in range(n):
        min_t = [F(wr.FMAX)] * 4
        key = [0] * 4
        inside_bit = [False] * 4
        in_sphere = False
        for s in range(S):
            T, dist, r2 = (F(v) for v in steps[s, i])
            sphere = 4 * int(gids[s >> 2]) + (s & 3)
            with np.errstate(invalid="ignore", over="ignore"):
                if simd:
                    L = s & 3
                    if not dist < r2:
                        continue  # HitMask
                    X = np.sqrt(F(r2 - dist))
                    t = F(T - X)
                    test = bool(t < eps)
                    if test:
                        t = F(T + X)
                    if not (t < min_t[L] and t > eps):
                        continue  # MoveMask
                    inside_bit[L] = inside_bit[L] or test
                    key[L] = sphere
                    min_t[L] = t
                else:
                    if dist > r2:
                        continue
                    X = np.sqrt(F(r2 - dist))
                    t = F(T - X)
                    test = bool(t < eps)
                    if test:
                        t = F(T + X)
                    if t > min_t[0]:
                        continue
                    if t < eps:
                        continue
                    in_sphere = test
                    key[0] = sphere
                    min_t[0] = t
        out[i, 0:4] = np.array(min_t, F).view(U)
        out[i, 4:8] = [k | (0x80000000 if b else 0) for k, b in zip(key, inside_bit)]
        out[i, 8] = int(in_sphere)
    return out


def random_steps(rng, n, S):
    """Steps drawn from a few values each, so that ties between classes and groups, inside hits (T < X), misses and
    it == eps happen in every lane's sequence; a few NaN dist among them."""
    T = rng.choice(np.array([-0.5, 0.0, 1e-4, 0.25, 0.5, 0.5, 1.0, 2.0], F), (S, n))
    r2 = rng.choice(np.array([0.25, 1.0, 4.0], F), (S, n))
    frac = rng.choice(np.array([0.0, 0.25, 0.75, 1.0, 1.5, np.nan], F), (S, n), p=[0.2, 0.25, 0.25, 0.1, 0.15, 0.05])
    return np.stack([T, (r2 * frac).astype(F), r2], 2).astype(F)


GIDS = np.array([0, 1, 2, 31, 100, 4095], U)  # 4095: rt_layout.h kMaxGroups - 1, so keys run from 0 to 16,383 | 2^31
MISS = (0.0, 2.0, 1.0)                         # dist > r2: no call under either rule set


def out_hit(v):
    """An outside hit at it == v exactly (dyadic v >= 2^-10): X = 1/4 from r2 = 1, dist = 15/16."""
    return (v + 0.25, 0.9375, 1.0)


def in_hit(v):
    """An inside hit at it == v exactly (dyadic v < 2): X = 1 from r2 = 4, dist = 3; T - X = v - 2 < eps."""
    return (v - 1.0, 3.0, 4.0)


def crafted_steps(n):
    """(steps (24, n, 3), the pattern of every lane): lane i runs pattern i % len(patterns), so the lanes of one
    wave alternate between inside hits, outside hits and no hit at all.  Step s = 4 gs + L goes to class L of group
    GIDS[gs]; a step not named is MISS."""
    eps = wr.EPS
    X = F(2.0 ** -16)                      # eps and eps + X are both multiples of 2^-37 below 2^-13: all sums exact
    r2e, de = F(2.0 ** -10), F(2.0 ** -10 - 2.0 ** -32)   # r2 - dist = X^2 exactly

    def at(v):  # it == v by the outside root
        T = F(v + X)
        assert F(T - X) == v
        return (T, de, r2e)
    lo, hi = F(2.0 ** -36), F(2.0 ** 60)
    patterns = {
        "two classes, equal t": {0: out_hit(1.0), 1: out_hit(1.0), 6: in_hit(1.0)},
        "two groups of one class, equal t": {0: out_hit(1.0), 4: out_hit(1.0), 13: in_hit(0.5), 17: out_hit(0.5)},
        "inside first, nearer outside later": {2: in_hit(1.5), 14: out_hit(0.5)},
        "outside first, nearer inside later": {2: out_hit(1.5), 14: in_hit(0.5)},
        "no hit": {},
        "around eps": {0: at(eps), 1: at(np.nextafter(eps, F(1))), 2: at(np.nextafter(eps, F(0))),
                       3: (F(eps - X), de, r2e)},                       # T - X < eps, T + X == eps
        "only eps": {20: at(eps)},
        "r2 - dist = 0 at the fast range's ends": {4: (0.5, lo, lo), 9: (0.25, hi, hi)},
        "r2 - dist = ulp(r2) / 2 at the fast range's ends": {
            4: (0.5, np.nextafter(lo, F(0)), lo), 9: (2.0 ** 18 + 1.0, np.nextafter(hi, F(0)), hi)},
        "one inside hit, largest key": {23: in_hit(0.75)},
        "one outside hit, key 0": {0: out_hit(0.75)},
        "one inside hit, key 1": {1: in_hit(0.75)},
        "NaN dist, then a later hit, then NaN": {5: (1.0, np.nan, 1.0), 9: out_hit(0.5), 12: (1.0, np.nan, 1.0),
                                                 19: out_hit(0.25)},
        "NaN dist last": {3: out_hit(0.5), 22: (2.0, np.nan, 4.0)},
        "NaN T": {7: (np.nan, 0.5, 1.0), 8: out_hit(1.0)},
    }
    names = list(patterns)
    steps = np.empty((4 * len(GIDS), n, 3), F)
    steps[:] = np.array(MISS, F)
    for i in range(n):
        for s, v in patterns[names[i % len(names)]].items():
            steps[s, i] = v
    return steps, [names[i % len(names)] for i in range(n)]


def test_crafted_steps_do_what_their_names_say():
    """The crafted sequences against the plain loop, and the outcomes their names promise, from the plain loop."""
    steps, names = crafted_steps(60)
    by = {nm: i for i, nm in reversed(list(enumerate(names)))}
    for simd in (True, False):
        want = plain_hit_loop(simd, steps, GIDS)
        got = wr.candidate_steps(simd, steps, GIDS).words()
        assert wr.same_bits(got[:, :4].view(F), want[:, :4].view(F))[2] == 0 and np.array_equal(got[:, 4:], want[:, 4:])
    sw, cw = plain_hit_loop(True, steps, GIDS), plain_hit_loop(False, steps, GIDS)
    one = F(1.0).view(U)
    i = by["two groups of one class, equal t"]
    assert sw[i, 0] == one and sw[i, 4] == 0 and cw[i, 4] == 4 * 100 + 1 and cw[i, 8] == 0  # earliest / latest
    assert sw[i, 5] == (4 * 31 + 1) | 0x80000000, "SIMD: the equal outside hit of a later group does not clear the flag"
    i = by["inside first, nearer outside later"]
    assert sw[i, 6] == (4 * 31 + 2) | 0x80000000 and cw[i, 4] == 4 * 31 + 2 and cw[i, 8] == 0  # sticky / not
    i = by["outside first, nearer inside later"]
    assert sw[i, 6] == (4 * 31 + 2) | 0x80000000 and cw[i, 8] == 1
    i = by["no hit"]
    assert np.all(sw[i, :4].view(F) == wr.FMAX) and not sw[i, 4:].any() and not cw[i, 4:].any()
    i = by["around eps"]
    eps = wr.EPS.view(U)
    assert sw[i, 0] == F(wr.FMAX).view(U) and sw[i, 1] == eps + 1 and sw[i, 2] >> 31 == 0 and sw[i, 6] >> 31 == 1
    assert sw[i, 3] == F(wr.FMAX).view(U), "T + X == eps is no hit under the SIMD rules"
    assert cw[i, 0] == eps and cw[i, 4] == 3 and cw[i, 8] == 1, "the scalar rules accept it == eps, the later one"
    i = by["only eps"]
    assert sw[i, 0] == F(wr.FMAX).view(U) and cw[i, 0] == eps and cw[i, 4] == 4 * 4095
    i = by["one inside hit, largest key"]
    assert sw[i, 7] == (4 * 4095 + 3) | 0x80000000 and cw[i, 4] == 4 * 4095 + 3 and cw[i, 8] == 1
    i = by["NaN dist, then a later hit, then NaN"]
    assert sw[i, 1] == F(0.5).view(U) and sw[i, 3] == F(0.25).view(U), "SIMD: a NaN dist is no hit"
    assert cw[i, 0] == F(0.25).view(U) and cw[i, 4] == 4 * 100 + 3, "scalar: every later sphere replaces a NaN minimum"
    i = by["NaN dist last"]
    assert np.isnan(cw[i, :1].view(F))[0] and cw[i, 4] == 4 * 4095 + 2 and cw[i, 8] == 0, "scalar: the NaN is accepted"


@pytest.mark.parametrize("simd", [True, False])
def test_vectorised_hit_update_against_a_plain_loop(simd):
    rng = np.random.default_rng(8)
    steps = random_steps(rng, 400, 24)
    gids = GIDS
    want = plain_hit_loop(simd, steps, gids)
    got = wr.candidate_steps(simd, steps, gids).words()
    t_ok = wr.same_bits(got[:, :4].view(F), want[:, :4].view(F))
    assert t_ok[2] == 0, t_ok
    assert np.array_equal(got[:, 4:], want[:, 4:])
    if simd:
        ins = got[:, 4:8] >> 31
        assert ins.any() and not ins.all() and len(np.unique(got[:, 4:8] & 0x7FFFFFFF)) > 8
        assert not got[:, 8].any(), "`ins` is dead under the SIMD rules"
    else:
        assert got[:, 8].any() and not got[:, 8].all()
        assert np.isnan(got[:, 0].view(F)).any(), "a NaN dist is accepted under the scalar rules and stays"
        assert np.all(got[:, 1:4].view(F) == wr.FMAX) and not got[:, 5:8].any(), "the scalar rules use slot 0 only"


def test_own_rule_and_thresholds_against_the_proofs_spellings():
    rng = np.random.default_rng(9)
    n = 20_000
    o = rng.normal(size=(n, 3)).astype(F)
    u = tpb.unit(rng.normal(size=(n, 3)))
    r = (10.0 ** rng.uniform(-2, 1, n)).astype(F)
    s = (o + u * (r * (1 + rng.choice([0.0, 1e-7, -1e-6, 1e-3], n)).astype(F))[:, None]).astype(F)
    d = tpb.unit(-u + rng.normal(size=(n, 3)) * (10.0 ** rng.uniform(-6, 0, (n, 1))) - u * rng.choice([0, -2], (n, 1)))
    rho = (r * r).astype(F)
    rho[::50], rho[1::50] = np.inf, np.nan
    sc = np.concatenate([s, rho[:, None]], 1).astype(F)
    c = [(s[:, k] - o[:, k]).astype(F) for k in range(3)]
    want = test_own_sphere_skip.own_rule(c[0], c[1], c[2], d[:, 0], d[:, 1], d[:, 2], rho)
    got = wr.own_rule(o, d, sc)
    assert np.array_equal(got, want) and got.sum() > n // 20 and (~got).sum() > n // 20
    assert not got[::50].any() and not got[1::50].any() and not wr.origin_near(o, d, sc)[:100:50].any()
    near = wr.origin_near(o, d, sc)
    assert near.sum() > n // 2 and (~near).sum() > 100
    # the per-lane thresholds
    e, T, cc = wr.prefilter(o, d, s)
    e2, T2, cc2 = tpb.prefilter(c[0], c[1], c[2], d[:, 0], d[:, 1], d[:, 2], with_cc=True)
    for x, y in ((e, e2), (T, T2), (cc, cc2)):
        assert np.array_equal(wr.bits(x), wr.bits(y))
    beta = (-r * F(1.5)).astype(F)
    assert np.array_equal(wr.bits(wr.member_thr(cc, rho)), wr.bits(tpb.threshold(rho, cc, True)))
    t, b = wr.cluster_thr(cc, rho, beta)
    assert wr.same_bits(t, tpb.cluster_threshold(rho, cc, True))[2] == 0
    assert wr.same_bits(b, tpb.behind_threshold(beta, cc, True))[2] == 0
    for srho, ymid, yhalf in ((0.5, 0.1, 0.2), (3.0, -1.0, 0.01)):
        dd, thr = wr.cluster_slab(cc, T, o[:, 1], d[:, 1], F(srho), F(ymid), F(yhalf))
        with np.errstate(invalid="ignore"):
            skip = np.abs(dd) > thr
        assert np.array_equal(skip, tpb.slab_skip(T, cc, o[:, 1], d[:, 1], srho, ymid, yhalf))
        assert skip.any() and not skip.all()
