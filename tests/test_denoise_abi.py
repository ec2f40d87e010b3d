"""CPU-side checks of rt_denoise's interface (no GPU needed): a C99 unit compiled against the header has
rt_denoise_desc's offsets and size and the three constants; the ctypes mirror agrees with the C compiler; both
symbols are in SIGNATURES and the library exports them; rt_denoise_defaults fills what the header documents; the
refusals, which need no device, return RT_EINVAL through the library itself; and the Python wrapper checks its
counts and widths before it calls."""
import ctypes
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_trace.h"
EINVAL = -22
OFFSETS = [("Size", 0), ("Width", 4), ("Height", 8), ("Iterations", 12), ("Flags", 16), ("NormalPower", 20),
           ("SigmaDepth", 24), ("SigmaColor", 28), ("Mean", 32), ("Hit", 40), ("Normal", 48), ("Albedo", 56), ("Out", 64),
           ("Scratch", 72), ("Rgba8", 80)]
DEFAULTS = dict(iterations=3, normal_power=2, sigma_depth=0.25, sigma_color=0.5)


def _cc():
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler (build() needs one too)"
    return cc


def _compile(tmp_path, body):
    src = tmp_path / "denoise_layout.c"
    src.write_text("#include <stddef.h>\n#include \"rt_trace.h\"\n" + body + "\n")
    return subprocess.run([_cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", str(HEADER.parent),
                           str(src)], capture_output=True, text=True)


# C99 has no _Static_assert: a negative array size is the failed assertion
def _assert(name, cond):
    return f"typedef char {name}[({cond}) ? 1 : -1];"


def test_c99_layout_and_constants(rt, tmp_path):
    lines = [_assert("size_desc", "sizeof(rt_denoise_desc) == 88")]
    lines += [_assert("off_" + n.lower(), f"offsetof(rt_denoise_desc, {n}) == {o}") for n, o in OFFSETS]
    lines += [_assert("c_demodulate", "RT_DENOISE_DEMODULATE == 1u"), _assert("c_pow", "RT_DENOISE_SRGB_POW == 2u"),
              _assert("c_pow_is_the_trace_flag", "RT_DENOISE_SRGB_POW == RT_FLAG_SRGB_POW"),
              _assert("c_max", "RT_DENOISE_MAX_ITERATIONS == 8u"),
              # the call as a C host writes it
              "int filter(const float *d_mean, const rt_first_hit *d_hit, const float *d_normal, float *d_out,",
              "           float *d_scratch, uint32_t *d_rgba8) {",
              "    rt_denoise_desc d;",
              "    if (rt_denoise_defaults(&d) != RT_OK) return -1;",
              "    d.Width = 1920; d.Height = 1080;",
              "    d.Mean = d_mean; d.Hit = d_hit; d.Normal = d_normal; d.Out = d_out; d.Scratch = d_scratch;",
              "    d.Rgba8 = d_rgba8;",
              "    return rt_denoise(&d, NULL);",
              "}"]
    r = _compile(tmp_path, "\n".join(lines))
    assert r.returncode == 0, r.stderr
    # a wrong value is caught (the check above is not vacuous)
    assert _compile(tmp_path, _assert("wrong_on_purpose", "offsetof(rt_denoise_desc, Mean) == 28")).returncode != 0
    assert _compile(tmp_path, _assert("wrong_on_purpose", "RT_DENOISE_MAX_ITERATIONS == 9u")).returncode != 0


def test_ctypes_mirror_agrees(rt):
    assert ctypes.sizeof(rt.RtDenoiseDesc) == 88
    assert [(n, getattr(rt.RtDenoiseDesc, n).offset) for n, _ in rt.RtDenoiseDesc._fields_] == OFFSETS
    assert (rt.DENOISE_DEMODULATE, rt.DENOISE_SRGB_POW, rt.DENOISE_MAX_ITERATIONS) == (1, 2, 8)
    code = HEADER.read_text()
    for name, value in (("RT_DENOISE_DEMODULATE", 1), ("RT_DENOISE_SRGB_POW", 2), ("RT_DENOISE_MAX_ITERATIONS", 8)):
        m = re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u" % name, code)
        assert m and int(m.group(1), 0) == value, name


def test_header_and_library_carry_the_entry_points(rt):
    code = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ws = lambda s: re.sub(r"\s+", r"\\s*", re.escape(s).replace(r"\ ", " "))  # noqa: E731
    assert re.search(ws("int rt_denoise(const rt_denoise_desc *desc, void *stream)"), code)
    assert re.search(ws("int rt_denoise_defaults(rt_denoise_desc *out)"), code)
    # after the first-hit block, as the interface grew
    assert code.index("int rt_trace_first_hit(") < code.index("int rt_denoise(") < code.index("rt_trace_last_info(")
    for name, n_args in (("rt_denoise", 2), ("rt_denoise_defaults", 1)):
        assert name in rt.SIGNATURES and len(rt.SIGNATURES[name][1]) == n_args
        assert rt.SIGNATURES[name][0] is ctypes.c_int and hasattr(rt.lib(), name)


def test_defaults(rt):
    L = rt.lib()
    d = rt.RtDenoiseDesc()
    ctypes.memset(ctypes.byref(d), 0xA5, ctypes.sizeof(d))
    assert L.rt_denoise_defaults(ctypes.byref(d)) == 0
    assert d.Size == 88 and (d.Width, d.Height, d.Flags) == (0, 0, 0)
    assert (d.Iterations, d.NormalPower, d.SigmaDepth, d.SigmaColor) == tuple(DEFAULTS.values())
    assert all(getattr(d, n) is None for n in ("Mean", "Hit", "Normal", "Albedo", "Out", "Scratch", "Rgba8"))
    assert rt.denoise_defaults() == DEFAULTS
    assert L.rt_denoise_defaults(None) == EINVAL and b"rt_denoise_defaults: NULL argument" in L.rt_last_error()
    # the header documents them
    text = HEADER.read_text()
    doc = text[text.index("int rt_denoise(const"):text.index("int rt_denoise_defaults(")]
    for word in ("Iterations = 3", "NormalPower = 2", "SigmaDepth = 0.25f", "SigmaColor = 0.5f"):
        assert word in doc, word


def _desc(rt, base, **kw):
    """A desc the library accepts up to the launch (never reached here: each case below is refused first)."""
    d = rt.RtDenoiseDesc(88, 64, 48, 3, 0, 2, 0.25, 0.5, base, base + 64, base + 128, base + 192, base + 256, base + 320,
                         base + 384)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_refusals_through_the_library(rt):
    """Every refusal comes before anything is enqueued, so it needs no device: the pointers are host addresses,
    compared and never followed."""
    L = rt.lib()
    buf = (ctypes.c_uint8 * 512)()
    base = (ctypes.addressof(buf) + 15) & ~15
    nan, inf = float("nan"), float("inf")
    cases = [(dict(Size=80), b"Size 80"), (dict(Width=0), b"bad image size"), (dict(Height=65537), b"bad image size"),
             (dict(Iterations=0), b"Iterations 0"), (dict(Iterations=9), b"Iterations 9"), (dict(Flags=4), b"unknown flags 0x4"),
             (dict(NormalPower=9), b"NormalPower 9"), (dict(SigmaDepth=-1.0), b"SigmaDepth"), (dict(SigmaDepth=nan), b"SigmaDepth"),
             (dict(SigmaColor=inf), b"SigmaColor"), (dict(SigmaColor=-inf), b"SigmaColor"), (dict(Mean=None), b"Mean is NULL"),
             (dict(Hit=None), b"Hit is NULL"), (dict(Out=None), b"Out is NULL"), (dict(Normal=None), b"Normal is NULL"),
             (dict(Albedo=None, Flags=1), b"Albedo is NULL"), (dict(Scratch=None), b"Scratch is NULL"),
             (dict(Mean=base + 8), b"Mean is not 16-byte"), (dict(Hit=base + 68), b"Hit is not 8-byte"),
             (dict(Normal=base + 132), b"Normal is not 16-byte"), (dict(Albedo=base + 200), b"Albedo is not 16-byte"),
             (dict(Out=base + 264), b"Out is not 16-byte"), (dict(Scratch=base + 328), b"Scratch is not 16-byte"),
             (dict(Rgba8=base + 386), b"Rgba8 is not 4-byte"), (dict(Out=base), b"Out is Mean"),
             (dict(Scratch=base), b"Scratch is Mean"), (dict(Scratch=base + 256), b"Scratch is Out")]
    for kw, text in cases:
        assert L.rt_denoise(ctypes.byref(_desc(rt, base, **kw)), None) == EINVAL, kw
        assert text in L.rt_last_error(), (kw, L.rt_last_error())
    assert L.rt_denoise(None, None) == EINVAL and b"rt_denoise: NULL argument" in L.rt_last_error()


def test_wrapper_checks_its_arguments(rt):
    buf = (ctypes.c_uint8 * 512)()
    base = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(width=64, height=48, mean_ptr=base, hit_ptr=base + 64, out_ptr=base + 256)
    for bad in (dict(iterations=0), dict(iterations=9), dict(iterations=1.5), dict(iterations=True), dict(iterations="3"),
                dict(normal_power=-1), dict(normal_power=9), dict(normal_power=2.0), dict(sigma_depth=-0.5),
                dict(sigma_depth=float("nan")), dict(sigma_color=float("inf")), dict(sigma_color="1"),
                dict(sigma_color=1e39), dict(sigma_depth=np.float64(-1e-9))):
        with pytest.raises(ValueError, match="denoise: "):
            rt.denoise(**ok, **bad)
    # what the wrapper lets through, the library refuses: the defaults want Scratch and Normal
    with pytest.raises(rt.RtError, match="Normal is NULL with NormalPower 2"):
        rt.denoise(**ok, scratch_ptr=base + 320)
    with pytest.raises(rt.RtError, match="Scratch is NULL with Iterations 3"):
        rt.denoise(**ok, normal_ptr=base + 128)
    with pytest.raises(rt.RtError, match="Albedo is NULL"):
        rt.denoise(**ok, iterations=np.int64(1), normal_power=0, demodulate=True)
    with pytest.raises(rt.RtError, match="Out is Mean"):
        rt.denoise(64, 48, base, base + 64, base, iterations=1, normal_power=0)
