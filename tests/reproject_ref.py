"""rt_reproject restated in numpy (not a test): the checker of tests/test_gpu_reproject.py and test_reproject_ref.py.

include/rt_trace.h defines the pass operation by operation; this file performs exactly those operations on float32
arrays, one array operation per listed operation, the four taps in the stated order, so that it yields the one set
of bits the definition has.  It shares nothing with the kernel: no C, no library call.  numpy's float32 +, -, *, /
and sqrt are the IEEE operations (denormals kept), and nothing here is a reduction whose order numpy chooses.

A camera is the 24-float record of rt.camera_floats / oracle.camera: CameraPosition 0:3, CameraX 8:11, CameraY
12:15, FilmCenter 16:19, FilmW 20, FilmH 21.

    host_constants(prev_cam, w, h)             -> fv (3,), ff, wf, hf, hw, hh: what the host forms once
    project(cam, prev_cam, key, t)             -> sx, sy, d, te (H, W) f32 and ok (H, W) bool: steps 2 to 5
    reproject(mean, key, t, cam, prev_cam, ..) -> (Out (H, W, 4) f32, OutCount (H, W) u32, Rgba8 (H, W) u32 or None)
"""
import numpy as np

F = np.float32
HIT_MISS = np.uint32(0xFFFFFFFF)
HIT_INSIDE = np.uint32(0x80000000)
SRGB_POW = 2
EPS = F(1e-4)


def dot3(a, b):
    """(a.x*b.x + a.y*b.y) + a.z*b.z on triples of arrays or scalars."""
    px, py, pz = a[0] * b[0], a[1] * b[1], a[2] * b[2]
    return (px + py) + pz


def normalize(v):
    """The reference's Normalize: v / sqrt(dot3(v, v)), the zero vector where the squared length is <= 1e-4."""
    l2 = dot3(v, v)
    keep = l2 > EPS
    ln = np.sqrt(l2)
    return [np.where(keep, c / ln, F(0.0)).astype(np.float32) for c in v]


def host_constants(prev_cam, w, h):
    c = np.asarray(prev_cam, np.float32)
    fv = [c[16 + i] - c[i] for i in range(3)]
    ff = dot3(fv, fv)
    wf, hf = F(w), F(h)
    hw, hh = wf * F(0.5), hf * F(0.5)
    out = dict(fv=np.array(fv, np.float32), ff=F(ff), wf=wf, hf=hf, hw=F(hw), hh=F(hh))
    assert all(type(out[k]) is np.float32 for k in ("ff", "wf", "hf", "hw", "hh"))
    return out


def direction(cam, w, h):
    """Step 2: the pixel-centre primary direction, three (H, W) f32 arrays."""
    c = np.asarray(cam, np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    fx = F(-1.0) + (xs.astype(np.float32) * F(2.0)) / F(w)
    fy = F(-1.0) + (ys.astype(np.float32) * F(2.0)) / F(h)
    kx = (fx * c[20]) * F(0.5)
    ky = (fy * c[21]) * F(0.5)
    p = [(c[16 + i] + kx * c[8 + i]) + ky * c[12 + i] for i in range(3)]
    return normalize([p[i] - c[i] for i in range(3)])


def project(cam, prev_cam, key, t):
    """Steps 2 to 5 for every pixel (the values of a miss are formed and never used)."""
    h, w = key.shape
    c, pc = np.asarray(cam, np.float32), np.asarray(prev_cam, np.float32)
    k = host_constants(pc, w, h)
    with np.errstate(all="ignore"):
        d3 = direction(c, w, h)
        x = [c[i] + d3[i] * t for i in range(3)]
        v = [x[i] - pc[i] for i in range(3)]
        u = dot3(v, [pc[8], pc[9], pc[10]])
        vv = dot3(v, [pc[12], pc[13], pc[14]])
        d = dot3(v, [k["fv"][0], k["fv"][1], k["fv"][2]])
        qx = (u / d) * k["ff"]
        qy = (vv / d) * k["ff"]
        sx = (((qx * F(2.0)) / pc[20]) + F(1.0)) * k["hw"]
        sy = (((qy * F(2.0)) / pc[21]) + F(1.0)) * k["hh"]
        te = np.sqrt(dot3(v, v))
        ok = (d > 0) & (sx >= F(-1.0)) & (sx < k["wf"]) & (sy >= F(-1.0)) & (sy < k["hf"])
    for a in (sx, sy, d, te):
        assert a.dtype == np.float32
    return dict(sx=sx, sy=sy, d=d, te=te, ok=ok)


def reproject(mean, key, t, cam, prev_cam, history=None, hist_key=None, hist_t=None, hist_count=None, *, frames=1,
              max_history, depth_tolerance=0.0, flags=0, encode=None):
    """(Out, OutCount, Rgba8).  history, hist_key, hist_t, hist_count: all None (no history) or all given.
    `encode`: a function (v4 (n, 4) f32, pow) -> (n,) u32, the RGBA8 encoding of a running mean (the tests pass the
    oracle's encode_rgba8); None: no Rgba8."""
    mean = np.asarray(mean, np.float32)
    h, w = key.shape
    assert mean.shape == (h, w, 4) and t.shape == (h, w) and t.dtype == np.float32 and key.dtype == np.uint32
    assert 1 <= frames <= max_history <= 0xFFFFFFFF
    out = mean.copy()
    count = np.full((h, w), frames, np.uint32)
    if history is not None:
        history = np.asarray(history, np.float32)
        assert history.shape == (h, w, 4) and hist_key.dtype == np.uint32 and hist_t.dtype == np.float32
        assert hist_count.dtype == np.uint32
        pr = project(cam, prev_cam, key, t)
        ok = pr["ok"] & (key != HIT_MISS)
        with np.errstate(all="ignore"):
            fsx, fsy = np.floor(pr["sx"]), np.floor(pr["sy"])
            ax, ay = pr["sx"] - fsx, pr["sy"] - fsy
            x0 = np.where(ok, fsx, F(0.0)).astype(np.int64)
            y0 = np.where(ok, fsy, F(0.0)).astype(np.int64)
            lim = F(depth_tolerance) * pr["te"]
            acc = [np.zeros((h, w), np.float32) for _ in range(3)]
            ws = np.zeros((h, w), np.float32)
            n = np.full((h, w), 0xFFFFFFFF, np.uint32)
            kept = np.zeros((h, w), bool)
            for iy, ix in ((0, 0), (0, 1), (1, 0), (1, 1)):
                qx, qy = x0 + ix, y0 + iy
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)  # (a clipped tap is not `inside`)
                wx = ax if ix else F(1.0) - ax
                wy = ay if iy else F(1.0) - ay
                wgt = wx * wy
                hq = history[qy, qx]
                take = ok & inside & (wgt > 0) & (hist_count[qy, qx] != 0) & (hist_key[qy, qx] == key)
                take = take & np.isfinite(hq[..., 0]) & np.isfinite(hq[..., 1]) & np.isfinite(hq[..., 2])
                if depth_tolerance > 0:
                    take = take & (np.abs(pr["te"] - hist_t[qy, qx]) <= lim)
                for ch in range(3):
                    acc[ch] = np.where(take, acc[ch] + wgt * hq[..., ch], acc[ch]).astype(np.float32)
                ws = np.where(take, ws + wgt, ws).astype(np.float32)
                n = np.where(take, np.minimum(n, hist_count[qy, qx]), n).astype(np.uint32)
                kept = kept | take
            n = np.minimum(n, np.uint32(max_history)).astype(np.uint32)
            a = F(frames) / (n.astype(np.float32) + F(frames))
            for ch in range(3):
                hc = acc[ch] / ws
                folded = hc + (mean[..., ch] - hc) * a
                assert folded.dtype == np.float32
                out[..., ch] = np.where(kept, folded, mean[..., ch])
            total = np.minimum(n.astype(np.uint64) + np.uint64(frames), np.uint64(max_history)).astype(np.uint32)
            count = np.where(kept, total, count).astype(np.uint32)
    rgba = None
    if encode is not None:
        rgba = encode(np.ascontiguousarray(out.reshape(-1, 4)), bool(flags & SRGB_POW)).reshape(h, w)
    return out, count, rgba
