"""The device math layer of csrc/rtk_math.h, each function alone, against references that do not come from the
GPU; and whole frames that take the trace kernels to the same edges.

tests/math_probe/libmath_probe.so (tests/math_probe/math_probe.hip, built by build() with the kernel units' own
flags) includes rtk_math.h itself and runs out[i] = f(in[i]); tests/math_probe.py loads it.  Every reference is
computed here in numpy or Python, and every comparison is of bit patterns.

"f64" below means: compute in float64, then round once to float32.  For sqrt, / and 1/x of float32 operands
that is the correctly rounded float32 result: float64 carries 53 >= 2 * 24 + 2 significant bits, and with that
many the second rounding cannot change the result of the first (double rounding is innocuous for these three
operations; Figueroa 1995).

What is held, and to what:
  sqrt_rn        np.sqrt in f64: every f32 of [1, 4) (both exponent parities), +0, and 4,096 mantissas of every
                 binade from 2^-102 to 2^127 in three named ranges (SQRT_RANGES), so that a failure says which
                 claim broke; for x < 0 the one property its only consumer needs (test_sqrt_rn_below_zero...)
  rcp_rn         f64 1/b
  div_rn         f64 a/b within its stated conditions (b > 0, a = +0 or |a/b| >= 2^-100)
  fold_weights   {RN(1/n), RN((f32)pc / n)}, n = (f32)(pc + 1) rounded to nearest even from u32
  normalize      the reference's sequence restated in numpy (normalize_ref), itself tied to the oracle's
                 or_normalize on the same inputs; classes a-g of NORMALIZE_CLASSES
  rsqrt_x86      the oracle's direct form restated in numpy, on every value of the bits it reads, two tables,
                 table in global memory and in LDS
  seed_mix, pcg  Python integers mod 2^64
  rand_float     float32(u) * inv + lo in float32 steps
  reflectance    exact rational arithmetic for the fused last step, rounded once to float32
  frames         tests/test_huge_sphere_frames.py's scenes (camera inside a sphere of radius 2^29 .. 2^63.99),
                 both rule sets, default lanes and 4 lanes per pixel, against the oracle bit for bit

Measured on an MI355X before the fix that came with these tests (profiles/math_layer_pytest_gpu.log holds the
run after it, 36 tests in 3.4 s): everything passed but normalize's class g.  sqrt_rn(+inf) is NaN
(v_rsq_f32(+inf) = +0, inf * 0), so normalize returned three NaNs for all 2,066 vectors of the class where the
reference returns +-0; normalize now sends a len that is not a finite value up to 2^40 to its IEEE path and takes
len from the IEEE sqrt there.  sqrt_rn gave -inf on all 61,441 negative inputs, NaN for -0, +inf and NaN, -inf
for -inf.  The frames passed before the fix too: at radius float32(2^63.99) the normal's |N|^2 is still finite.
Two mutations of a scratch copy of the header, each caught: sqrt_rn replaced by the raw v_sqrt_f32 fails the
four positive-range sqrt tests (2,535,452 of the 2^24 inputs of [1, 4) one ulp off); rsqrt_x86 without its
`^ 1024u` fails all four table tests on every input.
"""
import fractions

import numpy as np
import pytest

import math_probe
from test_gpu_parity import assert_same, gpu_render
from test_huge_sphere_frames import B, FRAMES, H, RADII, W, huge_sphere_scene, oracle_frame

pytestmark = pytest.mark.gpu

F, D, U32, U64 = np.float32, np.float64, np.uint32, np.uint64
NAMED_MANTISSAS = (0, 1, 2, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFE, 0x7FFFFF)
PER_BINADE = 4096


@pytest.fixture(scope="module", autouse=True)
def _device(torch_cuda):
    """The probes need a HIP device (and torch's HIP runtime loaded first: math_probe.lib())."""
    math_probe.lib()


# ----------------------------------------------------------------------------------------------- helpers
def bits(a):
    return np.ascontiguousarray(a).view(U32 if np.asarray(a).dtype.itemsize == 4 else U64)


def binades(exponents, rng):
    """PER_BINADE positive floats of every binade [2^e, 2^(e+1)), e in exponents (unbiased, normal): the named
    mantissas, the rest seeded random."""
    out = []
    for e in exponents:
        m = np.concatenate([np.array(NAMED_MANTISSAS, U32),
                            rng.integers(0, 1 << 23, PER_BINADE - len(NAMED_MANTISSAS), dtype=np.int64).astype(U32)])
        out.append((U32(e + 127) << U32(23)) | m)
    return np.concatenate(out).view(F)


def rn32(x):
    """One rounding from f64 to f32 (overflow to inf and underflow are the conversion's own)."""
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(x, D).astype(F)


def assert_bits(got, want, inputs, what):
    """Bitwise equality; on failure the first few offending inputs, got and wanted, in hex."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = bits(got).reshape(len(got), -1), bits(want).reshape(len(want), -1)
    bad = np.flatnonzero(np.any(g != w, axis=1))
    if bad.size:
        cols = [bits(np.asarray(c)).reshape(len(got), -1) for c in inputs]
        rows = ["in " + " ".join(f"{int(v):#x}" for c in cols for v in c[i]) + " got " +
                " ".join(f"{int(v):#x}" for v in g[i]) + " want " + " ".join(f"{int(v):#x}" for v in w[i])
                for i in bad[:6]]
        raise AssertionError(f"{what}: {bad.size} of {len(got)} differ; " + "; ".join(rows))


# ----------------------------------------------------------------------------------------------- sqrt_rn
def sqrt_ref(x):
    return rn32(np.sqrt(np.asarray(x, F).astype(D)))


def test_sqrt_rn_every_f32_of_1_to_4():
    """Every mantissa of [1, 2) and [2, 4): both exponent parities, 2^24 inputs."""
    x = np.arange(0x3F800000, 0x40800000, dtype=U32).view(F)
    assert x.size == 1 << 24 and x[0] == 1.0 and x[-1] < 4.0
    assert_bits(math_probe.sqrt(x), sqrt_ref(x), [x], "sqrt_rn on [1, 4)")


def test_sqrt_rn_of_zero_is_plus_zero():
    got = math_probe.sqrt(np.zeros(1, F))
    assert bits(got)[0] == 0, hex(int(bits(got)[0]))


# (claim, unbiased exponents of the binades, further single values)
SQRT_RANGES = {
    "header": ("rtk_math.h: exact for x in [2^-60, 2^60]", range(-60, 60), [2.0 ** 60]),
    "design": ("DESIGN.md: exact beyond the callers' ranges on every normal from 2^-102 up", range(-102, -60), []),
    "normalize": ("normalize's own use: |v|^2 from 2^60 to the top of f32", range(60, 128), []),
}


@pytest.mark.parametrize("name", list(SQRT_RANGES))
def test_sqrt_rn_sampled_binades(name):
    claim, exps, extra = SQRT_RANGES[name]
    x = np.concatenate([binades(exps, np.random.default_rng(1000 + len(exps))), np.array(extra, F)])
    if name == "normalize":
        assert x.max() == np.finfo(F).max
    assert_bits(math_probe.sqrt(x), sqrt_ref(x), [x], claim)


def test_sqrt_rn_below_zero_never_claims_total_internal_reflection():
    """x in [-2^-10, -2^-25]: what 1 - cos_t^2 reaches when cos_t is a few ulps past +-1.  The one consumer is
    `eta * sin_t > 1.0f` (shade, dielectric branch), which the reference's sqrtss answers with NaN, so the
    comparison is false there; it must be false here: s is NaN or s <= 0, for every eta the built-in and the
    random scenes use."""
    x = -np.concatenate([binades(range(-25, -10), np.random.default_rng(25)), np.array([2.0 ** -10], F)])
    assert x.min() == -F(2.0 ** -10) and x.max() == -F(2.0 ** -25)
    s = math_probe.sqrt(x)
    print("sqrt_rn on x < 0: NaN", int(np.isnan(s).sum()), "-inf", int(np.isneginf(s).sum()), "finite",
          int(np.isfinite(s).sum()), "max finite", s[np.isfinite(s)].max() if np.isfinite(s).any() else None)
    edge = np.array([-0.0, np.inf, -np.inf, np.nan], F)
    print("sqrt_rn(-0, +inf, -inf, NaN) =", [hex(int(v)) for v in bits(math_probe.sqrt(edge))])
    assert np.all(np.isnan(s) | (s <= 0)), ("a positive root of a negative number", x[~(np.isnan(s) | (s <= 0))][:6])
    with np.errstate(over="ignore", invalid="ignore"):
        for eta in (F(1.0) / F(2.4), F(1.0) / F(1.5), F(1.5), F(2.4)):
            cant = (eta * s) > F(1.0)
            assert not cant.any(), (float(eta), [hex(int(v)) for v in bits(x[cant][:6])])


# ----------------------------------------------------------------------------------------------- rcp_rn
def rcp_inputs():
    rng = np.random.default_rng(40)
    parts = [np.arange(0x3F800000, 0x40000000, dtype=U32).view(F),                  # every mantissa of [1, 2)
             binades(range(-40, 40), rng),
             np.arange(1, 70001, dtype=np.int64).astype(F)]
    ints = [2 ** k + d for k in range(0, 33) for d in range(-2, 3) if 2 ** k + d > 0]
    parts.append(np.array(ints, D).astype(F))                                       # (f32)(2^k + d), nearest even
    return np.concatenate(parts)


def test_rcp_rn():
    b = rcp_inputs()
    assert b.min() >= F(2.0 ** -40) and b.max() <= F(2.0 ** 40)
    assert_bits(math_probe.rcp(b), rn32(1.0 / b.astype(D)), [b], "rcp_rn on [2^-40, 2^40]")


# ----------------------------------------------------------------------------------------------- fold_weights / div_rn
def fold_inputs():
    rng = np.random.default_rng(77)
    named = [2 ** k + d for k in range(1, 33) for d in range(-3, 4)]
    pc = np.concatenate([np.arange(0, 70001, dtype=np.int64), np.clip(np.array(named, np.int64), 0, 2 ** 32 - 2),
                         np.minimum(rng.integers(0, 1 << 32, 1 << 20, dtype=np.int64), 2 ** 32 - 2)])
    return pc.astype(U32)


def u32_to_f32(u):
    """(f32)u as v_cvt_f32_u32 does it: nearest even (u is exact in f64, which then rounds once)."""
    return np.asarray(u, np.int64).astype(D).astype(F)


def test_fold_weights():
    pc = fold_inputs()
    n = u32_to_f32(pc.astype(np.int64) + 1)
    want = np.stack([rn32(1.0 / n.astype(D)), rn32(u32_to_f32(pc).astype(D) / n.astype(D))], axis=1)
    assert n.max() == F(2.0 ** 32) and (2 ** 24 + 1) in pc  # the conversion's rounding is in the set
    assert_bits(math_probe.fold(pc), want, [pc], "fold_weights")


def div_pairs():
    rng = np.random.default_rng(4100)
    pc = fold_inputs()
    a_parts, b_parts = [u32_to_f32(pc)], [u32_to_f32(pc.astype(np.int64) + 1)]
    # the film point's ((x + j) * 2) / W, in the kernel's own f32 steps
    for w in (1, 3, 96, 1920, 7680, 65535):
        reps = max(4, 32768 // w)
        x = np.tile(np.arange(w, dtype=np.int64).astype(F), reps)
        j = (F(-0.5) + rng.random(x.size).astype(F)).astype(F)
        j[:w] = F(-0.5)
        j[w:2 * w] = F(0.5) - F(2.0 ** -24)
        a_parts.append((x + j) * F(2.0))
        b_parts.append(np.full(x.size, w, F))
    # seeded pairs: b in [2^-8, 2^8), |a| in [2^-40, 2^24)
    n = 1 << 21
    b = ((rng.integers(127 - 8, 127 + 8, n, dtype=np.int64) << 23) | rng.integers(0, 1 << 23, n, dtype=np.int64))
    k16 = np.arange(n) % 16
    near = rng.integers(0, 256, n, dtype=np.int64)
    near = np.where(rng.random(n) < 0.5, near, 0x7FFFFF - near)
    b = np.where(k16 == 1, (b & ~0x7FFFFF) | near, b).astype(U32).view(F)  # mantissa within 255 of all 0s / all 1s
    a = ((rng.integers(127 - 40, 127 + 24, n, dtype=np.int64) << 23) |
         rng.integers(0, 1 << 23, n, dtype=np.int64)).astype(U32).view(F)
    # a = RN(k b) moved by -1, 0, +1 ulp, k odd: quotients next to representable values and to midpoints
    k = (2 * rng.integers(0, 1 << 11, n, dtype=np.int64) + 1).astype(D)
    kb = rn32(k * b.astype(D))
    kb = (bits(kb).astype(np.int64) + rng.integers(-1, 2, n, dtype=np.int64)).astype(U32).view(F)
    a = np.where(k16 == 2, kb, a)
    a = np.where(rng.random(n) < 0.5, a, -a)
    a_parts += [a, np.zeros(4096, F)]
    b_parts += [b, b[:4096]]
    return np.concatenate(a_parts), np.concatenate(b_parts)


def test_div_rn():
    a, b = div_pairs()
    assert 3_500_000 < a.size < 5_000_000
    q = a.astype(D) / b.astype(D)
    assert (b > 0).all() and np.all((bits(a) == 0) | (np.abs(q) >= 2.0 ** -100)), "outside div_rn's stated conditions"
    assert_bits(math_probe.div(a, b), rn32(q), [a, b], "div_rn(a, b, rcp_rn(b))")


# ----------------------------------------------------------------------------------------------- normalize
def normalize_ref(v):
    """v3::Normalize as the reference computes it: l2 = (x x + y y) + z z in f32, op by op; keep = l2 > 1e-4;
    len = the correctly rounded sqrt; each quotient the correctly rounded division; +0 where not kept."""
    v = np.asarray(v, F).reshape(-1, 3)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        l2 = (x * x + y * y) + z * z
        keep = l2 > F(1e-4)
        length = rn32(np.sqrt(l2.astype(D)))
        q = rn32(v.astype(D) / length.astype(D)[:, None])
    return np.where(keep[:, None], q, F(0.0)), l2, length


def _units(rng, n, floor=0.05):
    """n unit vectors (f64) with every component at least `floor` in magnitude."""
    u = rng.normal(size=(3 * n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u = u[np.all(np.abs(u) >= floor, axis=1)]
    assert len(u) >= n
    return u[:n]


def _landing(rng, target_len, wanted_bits, of, n=400000):
    """Vectors of length about target_len whose f32 l2 (of="l2") or len (of="len") lands on the given bit
    patterns; at most 64 per pattern, and every pattern must be found."""
    v = (_units(rng, n) * (target_len * (1.0 + rng.uniform(-3e-7, 3e-7, (n, 1))))).astype(F)
    _, l2, length = normalize_ref(v)
    val = bits(l2 if of == "l2" else length)
    keep = []
    for w in wanted_bits:
        hit = np.flatnonzero(val == w)
        assert hit.size, f"no vector whose {of} is {w:#x}"
        keep.append(hit[:64])
    return v[np.concatenate(keep)]


def normalize_classes():
    rng = np.random.default_rng(20260)
    signs = lambda n: rng.choice(np.array([-1.0, 1.0], F), (n, 3))
    perms = lambda rows: np.concatenate([np.asarray(rows, F)[:, p] for p in ([0, 1, 2], [1, 2, 0], [2, 0, 1])])
    out = {}
    # a. components in [-2, 2]
    out["a"] = np.concatenate([rng.uniform(-2, 2, (4096, 3)).astype(F),
                               perms([[1, 0, 0], [-1, 0, 0], [2, 2, 2], [-2, 2, -2], [2, 0, 0], [1, 1, 1]])])
    # b. l2 within 3 ulps either side of the 1e-4 threshold (== is not kept, the next float up is)
    thr = int(bits(np.array([1e-4], F))[0])
    out["b"] = _landing(rng, 1e-2, [thr + d for d in range(-3, 4)], "l2")
    # c. one and two components +-0; subnormal components beside a normal one
    c = rng.uniform(-2, 2, (3072, 3)).astype(F)
    c[:1024, 0] = rng.choice(np.array([0.0, -0.0], F), 1024)
    c[1024:2048, 1] = rng.choice(np.array([0.0, -0.0], F), 1024)
    c[1024:2048, 2] = rng.choice(np.array([0.0, -0.0], F), 1024)
    sub = rng.integers(1, 1 << 23, 1024, dtype=np.int64).astype(U32).view(F) * rng.choice(np.array([-1, 1], F), 1024)
    c[2048:, 2] = sub
    c[2560:, 0] = np.array([1, 0x7FFFFF] * 256, U32).view(F)  # the smallest and the largest subnormal
    out["c"] = np.concatenate([c, c[:, [2, 0, 1]]])
    # d. a quotient below 2^-99: (1, 2^-e, 0) and (1, 2^-e, 1/2) for e in 95..126, at several scales
    d = []
    for s in (1.0, 2.0 ** -12, 1.75, 2.0 ** 10, 3.0 * 2.0 ** 20):
        for e in range(95, 127):
            d += [[s, s * 2.0 ** -e, 0.0], [s, -s * 2.0 ** -e, 0.5 * s], [s * 2.0 ** -e, -s, s]]
    out["d"] = perms(d)
    # e. len from 2^39 to 2^41: random directions at lengths with the named mantissas, and len landing on
    #    2^40 itself and on its two neighbours (the fallback's edge is len > 2^40)
    lens = np.concatenate([binades([39, 40], np.random.default_rng(5))[[*range(8), *range(PER_BINADE, PER_BINADE + 8)]],
                           np.array([2.0 ** 41], F)]).astype(D)
    e = np.concatenate([(_units(rng, 128) * L).astype(F) for L in lens])
    p40 = int(bits(np.array([2.0 ** 40], F))[0])
    out["e"] = np.concatenate([e, _landing(rng, 2.0 ** 40, [p40 - 1, p40, p40 + 1], "len")])
    # f. l2 in (2^60, 2^127]
    k = rng.uniform(30.1, 63.4, (4096, 1))
    out["f"] = np.concatenate([(_units(rng, 4096, 0.0) * 2.0 ** k).astype(F) * signs(4096),
                               perms([[2.0 ** 31, 2.0 ** 30, 2.0 ** 30], [2.0 ** 63, 2.0 ** 62, -2.0 ** 62],
                                      [2.0 ** 63, 1.0, 0.0], [-2.0 ** 45, 2.0 ** 45, 2.0 ** 45]])])
    # g. l2 = +inf with finite components: one component in [2^64, 2^127], and three of 2^63.5
    big = (2.0 ** rng.uniform(64, 127.9, 2048)).astype(F)
    g = (rng.uniform(-1, 1, (2048, 3)) * 2.0 ** rng.uniform(-20, 60, (2048, 1))).astype(F)
    g[np.arange(2048), rng.integers(0, 3, 2048)] = big * rng.choice(np.array([-1, 1], F), 2048)
    h = F(2.0 ** 63.5)
    out["g"] = np.concatenate([g, perms([[h, h, h], [-h, h, -h], [2.0 ** 64, 0.0, -0.0], [np.finfo(F).max] * 3,
                                         [-2.0 ** 127, 1.0, -1.0], [2.0 ** 64, -2.0 ** 64, 2.0 ** 64]])])
    return out


NORMALIZE_CLASSES = ("a", "b", "c", "d", "e", "f", "g")


@pytest.fixture(scope="module")
def normalize_inputs():
    return normalize_classes()


@pytest.mark.parametrize("cls", NORMALIZE_CLASSES)
def test_normalize(orc, normalize_inputs, cls):
    v = np.ascontiguousarray(normalize_inputs[cls])
    want, l2, length = normalize_ref(v)
    # the class is what it says
    if cls == "b":
        assert (l2 <= F(1e-4)).any() and (l2 > F(1e-4)).any()
    if cls == "d":  # both sides of the 2^-99 edge, also where no component is zero (a zero takes the IEEE path anyway)
        m = np.abs(want[(l2 > F(1e-4)) & np.all(v != 0, axis=1)]).min(axis=1)
        assert (m < F(2.0 ** -99)).any() and (m >= F(2.0 ** -99)).any()
    if cls == "e":
        assert length.min() >= 0.999 * 2.0 ** 39 and length.max() <= 1.001 * 2.0 ** 41
        assert (length == F(2.0 ** 40)).any() and (length > F(2.0 ** 40)).any() and (length < F(2.0 ** 40)).any()
        assert (np.abs(want).min(axis=1) >= F(2.0 ** -99)).all()  # only len decides the path
    if cls == "f":
        assert l2.min() > 2.0 ** 60 and np.isfinite(l2).all()
    if cls == "g":
        assert np.isposinf(l2).all() and np.isfinite(v).all()
        assert np.array_equal(bits(want), bits(v) & U32(0x80000000))  # +-0 with the component's sign
    # the restatement is the oracle's own or_normalize
    L = orc.lib()
    ov = np.zeros_like(v)
    for i in range(len(v)):
        L.or_normalize(v.ctypes.data + 12 * i, ov.ctypes.data + 12 * i)
    assert_bits(want, ov, [v], f"class {cls}: numpy restatement against or_normalize")
    assert_bits(math_probe.normalize(v), want, [v], f"normalize, class {cls}")


# ----------------------------------------------------------------------------------------------- rsqrt_x86
def rsqrt_ref(table, x):
    """The oracle's direct form (rt_oracle.c or_rsqrt): entry (e & 1) * 1024 + mantissa[22:13], scaled by
    (e - (e & 1)) / 2, e the unbiased exponent."""
    u = bits(np.asarray(x, F)).astype(np.int64)
    e = ((u >> 23) & 0xFF) - 127
    par = e & 1
    base = bits(np.asarray(table, F))[par * 1024 + ((u >> 13) & 1023)].astype(np.int64)
    sh = (e - par) // 2  # (e - par is even)
    return ((base - (sh << 23)) & 0xFFFFFFFF).astype(U32).view(F)


def rsqrt_inputs():
    """Every value of bits 30..13 with a biased exponent 1..254 (the function reads nothing else), the low 13
    bits 0, all ones, and one seeded random value each."""
    rng = np.random.default_rng(13)
    top = np.arange(1 << 10, 255 << 10, dtype=np.int64) << 13
    low = [np.zeros(top.size, np.int64), np.full(top.size, 0x1FFF, np.int64), rng.integers(0, 0x2000, top.size)]
    return np.concatenate([top | l for l in low]).astype(U32).view(F)


@pytest.mark.parametrize("in_lds", [False, True], ids=["table_in_global", "table_in_lds"])
@pytest.mark.parametrize("which", ["builtin", "random"])
def test_rsqrt_x86(rt, orc, which, in_lds):
    x = rsqrt_inputs()
    assert x.size == 3 * 254 * 1024 and x.min() == np.finfo(F).tiny and np.isfinite(x).all()
    if which == "builtin":
        table = rt.rsqrt_table_builtin()
        # (the built-in table is the oracle's: tests/test_abi.py) the numpy form is or_rsqrt's
        L = orc.lib()
        sub = x[:: 97]
        assert_bits(rsqrt_ref(table, sub), np.array([L.or_rsqrt(float(v)) for v in sub], F), [sub], "rsqrt_ref against or_rsqrt")
    else:  # no two entries equal, so a wrong index cannot pass
        table = np.random.default_rng(2048).permutation(np.arange(0x3F000000, 0x40000000, 4099, dtype=U32))[:2048].view(F)
        assert table.size == 2048 and np.unique(table).size == 2048 and table.min() >= 0.5 and table.max() < 2.0
    assert_bits(math_probe.rsqrt(table, x, in_lds), rsqrt_ref(table, x), [x], f"rsqrt_x86, {which} table, in_lds={in_lds}")


# ----------------------------------------------------------------------------------------------- seed_mix, pcg, rand_float
M64 = (1 << 64) - 1


def seed_mix_int(i):
    """main.cpp:668-675 on Python integers."""
    s = (0x420247153476526 * i) & M64
    s = (s + 0x8442885C91A5C8D) & M64
    s ^= s >> ((7 + i) % 64)
    s ^= (s << 23) & M64
    s ^= s >> ((0x29 ^ i) % 64)
    s = (s * 0x11C19226CEB4769A + 0x1105404122082911) & M64
    s ^= (s << 19) & M64
    s ^= s >> 13
    return s


def pcg_int(s):
    """base.h:954-963 on Python integers: (value, new state)."""
    v = ((s >> 32) ^ s) & 0xFFFFFFFF
    r = s >> 59
    return ((v >> r) | (v << (32 - r))) & 0xFFFFFFFF, (s * 6364136223846793005 + 1442695040888963407) & M64


def pcg_np(s):
    """pcg_int on a uint64 array (wrapping arithmetic)."""
    s = np.asarray(s, U64)
    with np.errstate(over="ignore"):
        new = s * U64(6364136223846793005) + U64(1442695040888963407)
    v = ((s >> U64(32)) ^ s) & U64(0xFFFFFFFF)
    r = s >> U64(59)
    return (((v >> r) | (v << (U64(32) - r))) & U64(0xFFFFFFFF)).astype(U32), new


def state_for(u, r, rng):
    """A PCG state whose output is u through a rotation by r."""
    hi = (r << 27) | int(rng.integers(0, 1 << 27))
    v = ((u << r) | (u >> (32 - r))) & 0xFFFFFFFF  # rotate left: the output rotates it back
    return (hi << 32) | (hi ^ v)


def pcg_states():
    rng = np.random.default_rng(59)
    s = rng.integers(0, 1 << 64, 1 << 20, dtype=U64)
    top = rng.integers(0, 1 << 59, 512, dtype=U64)
    named = [state_for(u, r, rng) for u in (0, 1, (1 << 24) + 1, (1 << 32) - 1, 1 << 31) for r in (0, 1, 13, 31)]
    return np.concatenate([s, top[:256], top[256:] | (U64(31) << U64(59)), np.array(named, U64)])


def test_seed_mix():
    rng = np.random.default_rng(668)
    i = np.concatenate([np.arange(65536, dtype=U64),
                        np.array([(1 << 32) + d for d in range(-8, 9)] + [(1 << 63) + d for d in range(-8, 9)], U64),
                        rng.integers(0, 1 << 64, 1 << 17, dtype=U64)])
    ints = [int(v) for v in i]
    assert {(7 + v) % 64 for v in ints} == set(range(64)) and {(0x29 ^ v) % 64 for v in ints} == set(range(64))
    want = np.array([seed_mix_int(v) for v in ints], U64)
    assert_bits(math_probe.seed(i), want, [i], "seed_mix")


def test_pcg():
    s = pcg_states()
    assert set((s >> U64(59)).tolist()) == set(range(32))
    value, state = pcg_np(s)
    check = list(range(4096)) + list(range(len(s) - 600, len(s)))  # numpy's wrapping form is the integer form
    assert all(pcg_int(int(s[k])) == (int(value[k]), int(state[k])) for k in check)
    got_value, got_state = math_probe.pcg(s)
    assert_bits(got_value, value, [s], "pcg value")
    assert_bits(got_state, state, [s], "pcg state")


def test_rand_float():
    s = pcg_states()
    u, _ = pcg_np(s)
    assert {0, (1 << 24) + 1, (1 << 32) - 1} <= set(u[-20:].tolist())
    uf = u32_to_f32(u)
    got = math_probe.rand(s)
    for row, (lo, span) in enumerate(math_probe.RAND_RANGES):
        inv = F(span / 4294967295.0)  # RandomFloat's (Max - Min) / (f64)(u32)-1 rounded to f32
        want = (uf * inv).astype(F) + F(lo)
        assert_bits(got[row], want, [s], f"rand_float, lo {lo}, range {span}")


# ----------------------------------------------------------------------------------------------- reflectance
def round_fraction_to_f32(q):
    """The float32 nearest to the rational q, ties to even (one rounding)."""
    if q == 0:
        return F(0.0)
    sign, q = (-1.0, -q) if q < 0 else (1.0, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    e -= 1 if fractions.Fraction(2) ** e > q else 0     # 2^e <= q < 2^(e + 1)
    quantum = fractions.Fraction(2) ** (max(e, -126) - 23)
    n, rem = divmod(q, quantum)
    n = int(n)
    if 2 * rem > quantum or (2 * rem == quantum and n % 2 == 1):
        n += 1
    return F(sign * float(n * quantum))  # n < 2^25: n * quantum is exact in f64, and in f32 unless it overflows


def reflectance_inputs(rt):
    r0 = [F(0.0), F(0.04), F(1.0)]
    for index in (0, 1, 2):
        _, _, mats = rt.scene_arrays(rt.scene_builtin(index))
        for ior in np.unique(mats[:, 9][mats[:, 9] != 0]):  # both sides, the host's own f32 steps (rt_pack.cpp put_material)
            eo = F(1.0) / ior
            ro, ri = (F(1.0) - eo) / (F(1.0) + eo), (F(1.0) - ior) / (F(1.0) + ior)
            r0 += [ro * ro, ri * ri]
    r0 = np.unique(np.array(r0, F))
    one = F(1.0)
    edges = [0.0, -0.0, np.nextafter(F(0), one), np.nextafter(F(0), -one), np.finfo(F).tiny, -np.finfo(F).tiny,
             one, np.nextafter(one, F(0)), np.nextafter(one, F(2)), -one, np.nextafter(-one, F(0)), np.nextafter(-one, F(-2))]
    cos_t = np.concatenate([np.linspace(-1.0, 1.0, 20000 // len(r0)).astype(F), np.array(edges, F)])
    return np.repeat(cos_t, len(r0)), np.tile(r0, len(cos_t))


def test_reflectance(rt):
    cos_t, r0 = reflectance_inputs(rt)
    assert 15000 < cos_t.size < 25000 and np.unique(r0).size >= 5
    r1 = F(1.0) - cos_t
    r1 = r1 * r1 * r1 * r1 * r1                       # f32 products, left to right
    a = F(1.0) - r0
    fr = fractions.Fraction
    want = np.array([round_fraction_to_f32(fr(float(x)) * fr(float(y)) + fr(float(z))) for x, y, z in zip(a, r1, r0)], F)
    assert_bits(math_probe.refl(cos_t, r0), want, [cos_t, r0], "reflectance")


# ----------------------------------------------------------------------------------------------- whole frames
@pytest.fixture(scope="module")
def huge_frames(rt, orc):
    """(rt scene, the oracle's frame) per (radius name, rule set): rendered once, left unchanged."""
    cache = {}

    def get(radius, simd):
        if (radius, simd) not in cache:
            s, o = huge_sphere_scene(rt, orc, RADII[radius])
            cache[(radius, simd)] = (s, oracle_frame(orc, o, simd))
        return cache[(radius, simd)]
    return get


@pytest.mark.parametrize("simd", [True, False], ids=["simd", "scalar"])
@pytest.mark.parametrize("radius", list(RADII))
def test_frames_from_inside_a_huge_sphere(rt, torch_cuda, huge_frames, radius, simd):
    """48 x 32, 4 frames, 8 bounces from inside a sphere of radius 2^29 .. 2^63.99: running mean, RGBA8 and rays
    bit for bit (oracle_frame asserts that the oracle's frame has no NaN, no inf and no all-zero pixel, so no
    pixel is left out and no NaN rule is needed).  The short candidate sqrt's proof holds at 2^29 only."""
    s, ref = huge_frames(radius, simd)
    fast_sqrt = rt.scene_prefilter(s, simd)[2] & 2
    assert bool(fast_sqrt) == (radius == "2^29"), (radius, fast_sqrt)
    for lanes in (0, 4):
        d = rt.Device(0, options={"LanesPerPixel": lanes} if lanes else None)
        try:
            g = gpu_render(rt, torch_cuda, d, s, rt.camera_setup(s, W, H), W, H, frames=FRAMES, bounces=B, simd=simd)
            assert np.isfinite(g[0].cpu().numpy()).all(), f"LanesPerPixel {lanes}: NaN or inf in the GPU's running mean"
            assert_same(*g, *ref)
            if lanes:
                assert d.last_info()["LanesPerPixel"] == lanes, d.last_info()
        finally:
            d.close()
