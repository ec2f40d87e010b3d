"""rt_denoise restated in numpy (not a test): the checker of tests/test_gpu_denoise.py and test_denoise_ref.py.

include/rt_trace.h defines the filter operation by operation; this file performs exactly those operations on
float32 arrays, one array operation per listed operation, tap by tap in the stated order (dy outer, dx inner),
so that it yields the one set of bits the definition has.  It shares nothing with the kernel: no C, no library
call.  numpy's float32 +, -, *, / are the IEEE operations (denormals kept), and nothing here is a reduction
whose order numpy chooses.

    denoise(mean, hit_key, hit_t, ...) -> (out (H, W, 4) f32, rgba8 (H, W) u32)
    passes(...)                        -> the list of I_1 .. I_n before re-modulation (for the unit tests)
"""
import numpy as np

F = np.float32
K = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], dtype=np.float32)
HIT_MISS = np.uint32(0xFFFFFFFF)
DEMODULATE, SRGB_POW = 1, 2
LUM = (F(0.2126), F(0.7152), F(0.0722))


def lum(c):
    return (LUM[0] * c[..., 0] + LUM[1] * c[..., 1]) + LUM[2] * c[..., 2]


def pos(v):
    """v > 0 ? v : 0 (a NaN gives 0)."""
    return np.where(v > 0, v, F(0.0)).astype(np.float32)


def host_ic(sigma_color, n):
    """ic0 = 1.0f / SigmaColor once, then ic = ic0 * (float)(1 << i) per pass."""
    ic0 = F(1.0) / F(sigma_color)
    return [F(ic0 * F(1 << i)) for i in range(n)]


def albedo_divisor(albedo):
    """a (H, W, 3): Albedo.ch > 0.01f ? Albedo.ch : 0.01f where Albedo.w == 1, and 1 on a miss."""
    a = np.where(albedo[..., :3] > F(0.01), albedo[..., :3], F(0.01)).astype(np.float32)
    return np.where((albedo[..., 3] == F(1.0))[..., None], a, F(1.0)).astype(np.float32)


def one_pass(img, key, t, normal, step, normal_power, sigma_depth, ic):
    """I_{i+1} (H, W, 3) from I_i (H, W, 3) at `step`; ic None: no colour stop."""
    h, w = key.shape
    s = int(step)
    surface = key != HIT_MISS
    lp = lum(img) if ic is not None else None
    if sigma_depth > 0:
        with np.errstate(all="ignore"):
            rz = (F(1.0) / (F(sigma_depth) * t)).astype(np.float32)  # (used where the centre is a hit)
    acc = np.zeros((h, w, 3), np.float32)
    ws = np.zeros((h, w), np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * s, xs + dx * s
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)  # (a clipped tap is not `inside`)
                wgt = np.full((h, w), K[dy + 2] * K[dx + 2], np.float32)
                take = inside
                iq = img[qy, qx]
                if dx != 0 or dy != 0:
                    take = take & (key[qy, qx] == key)
                    if normal_power > 0:
                        nq = normal[qy, qx]
                        px, py, pz = normal[..., 0] * nq[..., 0], normal[..., 1] * nq[..., 1], normal[..., 2] * nq[..., 2]
                        d = pos((px + py) + pz)
                        for _ in range(int(normal_power)):
                            d = d * d
                        wgt = np.where(surface, wgt * d, wgt).astype(np.float32)
                    if sigma_depth > 0:
                        f = pos(F(1.0) - np.abs(t - t[qy, qx]) * rz)
                        wgt = np.where(surface, wgt * f, wgt).astype(np.float32)
                    if ic is not None:
                        wgt = wgt * pos(F(1.0) - np.abs(lp - lp[qy, qx]) * F(ic))
                    take = take & (wgt > 0)
                for ch in range(3):
                    acc[..., ch] = np.where(take, acc[..., ch] + wgt * iq[..., ch], acc[..., ch])
                ws = np.where(take, ws + wgt, ws).astype(np.float32)
        out = np.empty((h, w, 3), np.float32)
        for ch in range(3):
            out[..., ch] = acc[..., ch] / ws
    assert out.dtype == np.float32 and ws.dtype == np.float32 and acc.dtype == np.float32
    return out


def passes(mean, key, t, normal=None, albedo=None, *, iterations, normal_power=0, sigma_depth=0.0, sigma_color=0.0,
           flags=0):
    """[I_1, ..., I_n], each (H, W, 3) f32: before the demodulated variant multiplies back."""
    mean = np.asarray(mean, np.float32)
    h, w = key.shape
    assert mean.shape == (h, w, 4) and t.shape == (h, w) and t.dtype == np.float32 and key.dtype == np.uint32
    img = mean[..., :3].copy()
    if flags & DEMODULATE:
        with np.errstate(all="ignore"):
            img = (img / albedo_divisor(albedo)).astype(np.float32)
    ics = host_ic(sigma_color, iterations) if sigma_color > 0 else [None] * iterations
    out = []
    for i in range(iterations):
        img = one_pass(img, key, t, normal, 1 << i, normal_power, F(sigma_depth), ics[i])
        out.append(img)
    return out


def denoise(mean, key, t, normal=None, albedo=None, *, iterations, normal_power=0, sigma_depth=0.0, sigma_color=0.0,
            flags=0, encode=None):
    """(Out (H, W, 4) f32, Rgba8 (H, W) u32 or None).  `encode`: a function (v4 (n, 4) f32, pow) -> (n,) u32, the
    RGBA8 encoding of a running mean (the tests pass the oracle's encode_rgba8: main.cpp:312-346); None: no Rgba8."""
    img = passes(mean, key, t, normal, albedo, iterations=iterations, normal_power=normal_power, sigma_depth=sigma_depth,
                 sigma_color=sigma_color, flags=flags)[-1]
    if flags & DEMODULATE:
        with np.errstate(all="ignore"):
            img = (img * albedo_divisor(albedo)).astype(np.float32)
    out = np.concatenate([img, np.asarray(mean, np.float32)[..., 3:4]], axis=2)
    rgba = None
    if encode is not None:
        rgba = encode(np.ascontiguousarray(out.reshape(-1, 4)), bool(flags & SRGB_POW)).reshape(key.shape)
    return out, rgba
