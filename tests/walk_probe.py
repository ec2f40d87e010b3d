"""ctypes loader of tests/walk_probe/libwalk_probe.so (test helper): the walk layer of csrc/rtk_walk.h, one function
or small family per call, alone on the GPU (tests/walk_probe/walk_probe.hip includes the header itself; the library
is built by __graft_entry__.build() with the kernel translation units' own flags).

Every function takes and returns numpy arrays.  `early` picks how the lanes past the count behave (0: they compute on
a clamped index and store nothing; 1: they return first, so the last wave runs under partial exec).  Every output
buffer has tests/sched_probe.py's guard words behind it, checked when it is read back."""
import ctypes
import pathlib

import numpy as np

from sched_probe import Buf

LIB_PATH = pathlib.Path(__file__).resolve().parent / "walk_probe" / "libwalk_probe.so"
F, U = np.float32, np.uint32
_L = None
FILL = 0xCD  # every output starts as this byte: a word the kernel did not store shows


def lib() -> ctypes.CDLL:
    global _L
    if _L is None:
        if not LIB_PATH.exists():
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build()")
        import torch  # noqa: F401  (one HIP runtime per process: tests/math_probe.py's rule)
        L = ctypes.CDLL(str(LIB_PATH))
        v, u32, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
        for name, args in (("exact", [v, u32, v, u32, u32, i, v, v]),
                           ("candidate", [v, v, u32, u32, i, i, i, v, v]),
                           ("group", [v, u32, v, u32, u32, v, u32, i, i, i, i, v, v]),
                           ("prefilter", [v, u32, v, u32, i, v, v]),
                           ("prefilter_group", [v, u32, v, u32, i, i, v, v]),
                           ("expand", [v, u32, v, i, v, v]),
                           ("prefilter_x", [v, u32, v, v, u32, i, v, v]),
                           ("thresholds", [v, v, u32, v, u32, i, v, v]),
                           ("own", [v, v, v, u32, i, v, v])):
            fn = getattr(L, "walk_probe_" + name)
            fn.restype = i
            fn.argtypes = args
        _L = L
    return _L


def _run(name, out_shape, out_dtype, make_args):
    """Allocates the output (guarded, prefilled), calls walk_probe_<name>(*make_args(out pointer, stream)), reads back."""
    import torch
    L = lib()
    out = Buf(np.full(out_shape, FILL * 0x01010101, U).view(out_dtype))
    stream = torch.cuda.current_stream().cuda_stream
    rc = getattr(L, "walk_probe_" + name)(*make_args(out.ptr, stream))
    torch.cuda.synchronize()
    if rc != 0:
        raise RuntimeError(f"walk_probe_{name} failed ({rc})")
    return out.read()


def _rays(o, d):
    r = np.ascontiguousarray(np.concatenate([np.asarray(o, F), np.asarray(d, F)], axis=1), F)
    assert r.ndim == 2 and r.shape[1] == 6
    return Buf(r), len(r)


def pair_table(centres):
    """Two rows per sphere pair, {x0, x1, y0, y1} and {z0, z1, 0, 0}, of centres (2 m, 3)."""
    c = np.asarray(centres, F).reshape(-1, 2, 3)
    t = np.zeros((len(c), 2, 4), F)
    t[:, 0, 0:2], t[:, 0, 2:4], t[:, 1, 0:2] = c[:, :, 0], c[:, :, 1], c[:, :, 2]
    return t


def exact(o, d, centres, which, early):
    """(T, dist), each (n, 2 m), of which = 'core' (sphere_core), 'pair' (pair_dist) or 'c' (pair_dist_c: `centres`
    then holds the rows C = RN(S - O) of the common origin) over the m pairs of centres (2 m, 3)."""
    rays, n = _rays(o, d)
    tab = Buf(pair_table(centres))
    m = len(tab.host)
    w = {"core": 0, "pair": 1, "c": 2}[which]
    out = _run("exact", (m, n, 4), F, lambda p, s: (rays.ptr, n, tab.ptr, m, w, int(early), p, s))
    T = out[:, :, 0:2].transpose(1, 0, 2).reshape(n, 2 * m)
    dist = out[:, :, 2:4].transpose(1, 0, 2).reshape(n, 2 * m)
    return T, dist


def candidate(steps, gids, simd, fast, early):
    """The Hit words (n, 9) after steps (S, n, 3) of {T, dist, r2}; gids (S / 4,) group indices."""
    steps = np.ascontiguousarray(steps, F)
    S, n, _ = steps.shape
    gids = np.ascontiguousarray(gids, U)
    assert S == 4 * len(gids)
    st, gt = Buf(steps), Buf(gids)
    return _run("candidate", (n, 9), U,
                lambda p, s: (st.ptr, gt.ptr, n, len(gids), int(simd), int(fast), int(early), p, s))


VARIANTS = {"test_group": 0, "recheck00": 1, "recheck10": 2, "recheck01": 3, "recheck11": 4, "pf": 5, "prim": 6}


def group(o, d, groups, n_spheres, variant, simd, fast, early, rel=False, prim=None):
    """The Hit words (n, 9) of one of VARIANTS over packed group records (G, 5, 4); prim (G, 4, 4) for 'prim'."""
    rays, n = _rays(o, d)
    groups = np.ascontiguousarray(groups, F)
    assert groups.shape[1:] == (5, 4)
    gt = Buf(groups)
    pt = Buf(np.ascontiguousarray(prim, F)) if prim is not None else None
    assert (variant == "prim") == (prim is not None) and (prim is None or pt.host.shape == (len(groups), 4, 4))
    return _run("group", (n, 9), U,
                lambda p, s: (rays.ptr, n, gt.ptr, len(groups), n_spheres, pt.ptr if pt else None, VARIANTS[variant],
                              int(simd), int(fast), int(rel), int(early), p, s))


def prefilter(o, d, centres, early):
    """(e, T, cc), each (n, 2 m), of pair_prefilter."""
    rays, n = _rays(o, d)
    tab = Buf(pair_table(centres))
    m = len(tab.host)
    out = _run("prefilter", (m, n, 6), F, lambda p, s: (rays.ptr, n, tab.ptr, m, int(early), p, s))
    return tuple(out[:, :, 2 * k:2 * k + 2].transpose(1, 0, 2).reshape(n, 2 * m) for k in range(3))


def prefilter_group(o, d, groups, rel, early):
    """(n, G) words f01 | f23 << 1 of prefilter_group<REL>."""
    rays, n = _rays(o, d)
    gt = Buf(np.ascontiguousarray(groups, F))
    G = len(gt.host)
    out = _run("prefilter_group", (G, n), U, lambda p, s: (rays.ptr, n, gt.ptr, G, int(rel), int(early), p, s))
    return out.T.copy()


def _c0(c0):
    return Buf(np.array([c0[0], c0[1], c0[2], 0.0], F))


def expand(o, d, c0, early):
    """RayX (n, 8) of ray_expand."""
    rays, n = _rays(o, d)
    ct = _c0(c0)
    return _run("expand", (n, 8), F, lambda p, s: (rays.ptr, n, ct.ptr, int(early), p, s))


def prefilter_x(o, d, c0, centres, early):
    """(e', T), each (n, 2 m), of pair_prefilter_x on ray_expand's RayX against recentred centres (2 m, 3)."""
    rays, n = _rays(o, d)
    ct, tab = _c0(c0), Buf(pair_table(centres))
    m = len(tab.host)
    out = _run("prefilter_x", (m, n, 4), F, lambda p, s: (rays.ptr, n, ct.ptr, tab.ptr, m, int(early), p, s))
    return tuple(out[:, :, 2 * k:2 * k + 2].transpose(1, 0, 2).reshape(n, 2 * m) for k in range(2))


def thresholds(o, d, cc, T, entries, early):
    """cc, T (n, 2); entries (E, 3, 4): {r0, r1, beta0, beta1}, {srho0, srho1, ymid0, ymid1}, {yhalf0, yhalf1, -, -}.
    Returns a dict of (n, E, 2) arrays: member_t, cluster_t, cluster_b, slab_d, slab_thr."""
    rays, n = _rays(o, d)
    cct = Buf(np.ascontiguousarray(np.concatenate([cc, T], axis=1), F))
    et = Buf(np.ascontiguousarray(entries, F))
    E = len(et.host)
    assert cct.host.shape == (n, 4) and et.host.shape == (E, 3, 4)
    out = _run("thresholds", (E, n, 10), F, lambda p, s: (rays.ptr, cct.ptr, n, et.ptr, E, int(early), p, s))
    out = out.transpose(1, 0, 2)
    names = ("member_t", "cluster_t", "cluster_b", "slab_d", "slab_thr")
    return {k: out[:, :, 2 * j:2 * j + 2].copy() for j, k in enumerate(names)}


def own(o, d, sc, slot, early):
    """(own_sphere (n,) u32, origin_near (n,) bool) for sc (n, 4) = {S, rho} and slot (n,)."""
    rays, n = _rays(o, d)
    st, sl = Buf(np.ascontiguousarray(sc, F)), Buf(np.ascontiguousarray(slot, U))
    assert st.host.shape == (n, 4) and sl.host.shape == (n,)
    out = _run("own", (n, 2), U, lambda p, s: (rays.ptr, st.ptr, sl.ptr, n, int(early), p, s))
    return out[:, 0].copy(), out[:, 1] != 0
