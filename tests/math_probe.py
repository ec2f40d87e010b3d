"""ctypes loader of tests/math_probe/libmath_probe.so (test helper): the functions of csrc/rtk_math.h, each run
alone and element-wise on the GPU (tests/math_probe/math_probe.hip includes the header itself; the library is
built by __graft_entry__.build() with the kernel translation units' own flags).  Every function here takes and
returns numpy arrays; a negative code from the library raises."""
import ctypes
import pathlib

import numpy as np

LIB_PATH = pathlib.Path(__file__).resolve().parent / "math_probe" / "libmath_probe.so"
_L = None


def lib() -> ctypes.CDLL:
    global _L
    if _L is None:
        if not LIB_PATH.exists():
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build()")
        import torch  # noqa: F401  (one HIP runtime per process: the same rule as the package's lib())
        L = ctypes.CDLL(str(LIB_PATH))
        v, u32, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
        for name, args in (("sqrt", [v, v, u32]), ("rcp", [v, v, u32]), ("div", [v, v, v, u32]),
                           ("refl", [v, v, v, u32]), ("fold", [v, v, u32]), ("normalize", [v, v, u32]),
                           ("rsqrt", [v, v, v, u32, i]), ("seed", [v, v, u32]), ("pcg", [v, v, v, u32]),
                           ("rand", [v, v, u32])):
            fn = getattr(L, "math_probe_" + name)
            fn.restype = ctypes.c_int
            fn.argtypes = args
        _L = L
    return _L


def _in(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def _call(name, *args):
    rc = getattr(lib(), "math_probe_" + name)(*args)
    if rc != 0:
        raise RuntimeError(f"math_probe_{name} failed ({rc})")


def _unary(name, x, in_dtype, out_dtype, out_per_in=1):
    x = _in(x, in_dtype)
    out = np.empty(x.size * out_per_in, out_dtype)
    _call(name, x.ctypes.data, out.ctypes.data, x.size)
    return out


def _binary(name, a, b):
    a, b = _in(a, np.float32), _in(b, np.float32)
    assert a.size == b.size
    out = np.empty(a.size, np.float32)
    _call(name, a.ctypes.data, b.ctypes.data, out.ctypes.data, a.size)
    return out


def sqrt(x):
    """sqrt_rn(x)"""
    return _unary("sqrt", x, np.float32, np.float32)


def rcp(b):
    """rcp_rn(b)"""
    return _unary("rcp", b, np.float32, np.float32)


def div(a, b):
    """div_rn(a, b, rcp_rn(b))"""
    return _binary("div", a, b)


def refl(cos_t, r0):
    """reflectance(cos_t, r0)"""
    return _binary("refl", cos_t, r0)


def fold(pc):
    """fold_weights(pc) as an (n, 2) array"""
    return _unary("fold", pc, np.uint32, np.float32, 2).reshape(-1, 2)


def normalize(v):
    """normalize(x, y, z) of an (n, 3) array"""
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    out = np.empty_like(v)
    _call("normalize", v.ctypes.data, out.ctypes.data, len(v))  # (the count is of vectors, not of floats)
    return out


def rsqrt(table, x, in_lds: bool):
    """rsqrt_x86 with the caller's 2048-entry table, read from global memory or from the block's LDS copy"""
    table, x = _in(table, np.float32), _in(x, np.float32)
    assert table.size == 2048
    out = np.empty(x.size, np.float32)
    _call("rsqrt", table.ctypes.data, x.ctypes.data, out.ctypes.data, x.size, 1 if in_lds else 0)
    return out


def seed(i):
    """seed_mix(i)"""
    return _unary("seed", i, np.uint64, np.uint64)


def pcg(s):
    """(pcg(s), s afterwards)"""
    s = _in(s, np.uint64)
    value, state = np.empty(s.size, np.uint32), np.empty(s.size, np.uint64)
    _call("pcg", s.ctypes.data, value.ctypes.data, state.ctypes.data, s.size)
    return value, state


RAND_RANGES = ((-0.5, 1.0), (-1.0, 2.0), (0.0, 1.0))  # (lo, hi - lo) of the three planes, in order


def rand(s):
    """rand_float(s, lo, inv) as a (3, n) array, one row per entry of RAND_RANGES"""
    s = _in(s, np.uint64)
    return _unary("rand", s, np.uint64, np.float32, 3).reshape(3, -1)
