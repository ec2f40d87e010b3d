"""rt_reproject_clip restated in numpy (not a test): the checker of tests/test_gpu_reproject_clip.py and
test_reproject_clip_ref.py.

include/rt_trace.h defines the call as rt_reproject's steps 1 to 8 with one step (7a to 7d) between "H.ch = acc.ch /
ws" and the fold.  Steps 2 to 5 are tests/reproject_ref.py's project (with its host_constants and direction); steps 6
and 7 are restated here with the new step, one array operation per listed operation, the window's taps in the stated
order (dy outer, dx inner), so that the file yields the one set of bits the definition has.  It shares nothing with
the kernel.

    band(mean, key, radius, gamma)  -> lo, hi (H, W, 3) f32 and nf (H, W) f32: steps 7a to 7c for every pixel
    clamp(h, lo, hi, nf)            -> step 7d on one channel: by comparisons, a NaN bound clamps nothing
    reproject_clip(mean, key, t, cam, prev_cam, ..., radius, gamma)
                                    -> (Out (H, W, 4) f32, OutCount (H, W) u32, Rgba8 (H, W) u32 or None)
"""
import numpy as np

import reproject_ref as rr
from denoise_ref import pos

F = np.float32
HIT_MISS, HIT_INSIDE, SRGB_POW = rr.HIT_MISS, rr.HIT_INSIDE, rr.SRGB_POW


def band(mean, key, radius, gamma):
    """Steps 7a to 7c: the sums over the (2 * radius + 1)^2 window of the fresh planes and the band.  lo and hi are
    formed for every pixel; where nf == 0 they are 0 / 0 and never used."""
    mean = np.asarray(mean, np.float32)
    h, w = key.shape
    r = int(radius)
    assert 1 <= r <= 3 and mean.shape == (h, w, 4) and key.dtype == np.uint32
    g = F(gamma)
    ys, xs = np.mgrid[0:h, 0:w]
    s1 = [np.zeros((h, w), np.float32) for _ in range(3)]
    s2 = [np.zeros((h, w), np.float32) for _ in range(3)]
    nf = np.zeros((h, w), np.float32)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                qx, qy = xs + dx, ys + dy
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)  # (a clipped tap is not `inside`)
                c = mean[qy, qx]
                take = inside & (key[qy, qx] == key)
                take = take & np.isfinite(c[..., 0]) & np.isfinite(c[..., 1]) & np.isfinite(c[..., 2])
                for ch in range(3):
                    s1[ch] = np.where(take, s1[ch] + c[..., ch], s1[ch]).astype(np.float32)
                    sq = c[..., ch] * c[..., ch]
                    s2[ch] = np.where(take, s2[ch] + sq, s2[ch]).astype(np.float32)
                nf = np.where(take, nf + F(1.0), nf).astype(np.float32)
        lo = np.zeros((h, w, 3), np.float32)
        hi = np.zeros((h, w, 3), np.float32)
        for ch in range(3):
            m = s1[ch] / nf
            e2 = s2[ch] / nf
            mm = m * m
            v = pos(e2 - mm)
            sd = np.sqrt(v)
            gs = g * sd
            lo[..., ch] = m - gs
            hi[..., ch] = m + gs
            for a in (m, e2, mm, v, sd, gs):
                assert a.dtype == np.float32
    return lo, hi, nf


def clamp(hc, lo, hi, nf):
    """Step 7d on one channel: if (H < lo) H = lo; if (H > hi) H = hi; where nf > 0."""
    with np.errstate(invalid="ignore"):
        out = np.where((nf > 0) & (hc < lo), lo, hc).astype(np.float32)
        out = np.where((nf > 0) & (out > hi), hi, out).astype(np.float32)
    return out


def reproject_clip(mean, key, t, cam, prev_cam, history=None, hist_key=None, hist_t=None, hist_count=None, *, frames=1,
                   max_history, depth_tolerance=0.0, flags=0, encode=None, radius, gamma):
    """(Out, OutCount, Rgba8): tests/reproject_ref.py reproject's arguments and `radius`, `gamma`."""
    mean = np.asarray(mean, np.float32)
    h, w = key.shape
    assert mean.shape == (h, w, 4) and t.shape == (h, w) and t.dtype == np.float32 and key.dtype == np.uint32
    assert 1 <= frames <= max_history <= 0xFFFFFFFF
    assert 1 <= int(radius) <= 3 and np.isfinite(F(gamma)) and F(gamma) > 0
    out = mean.copy()
    count = np.full((h, w), frames, np.uint32)
    if history is not None:
        history = np.asarray(history, np.float32)
        assert history.shape == (h, w, 4) and hist_key.dtype == np.uint32 and hist_t.dtype == np.float32
        assert hist_count.dtype == np.uint32
        pr = rr.project(cam, prev_cam, key, t)
        ok = pr["ok"] & (key != HIT_MISS)
        lo, hi, nf = band(mean, key, radius, gamma)
        with np.errstate(all="ignore"):
            # step 6, as tests/reproject_ref.py has it
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
                qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
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
            # step 7 with 7a to 7d between H and the fold
            n = np.minimum(n, np.uint32(max_history)).astype(np.uint32)
            a = F(frames) / (n.astype(np.float32) + F(frames))
            for ch in range(3):
                hc = acc[ch] / ws
                hc = clamp(hc, lo[..., ch], hi[..., ch], nf)
                folded = hc + (mean[..., ch] - hc) * a
                assert folded.dtype == np.float32
                out[..., ch] = np.where(kept, folded, mean[..., ch])
            total = np.minimum(n.astype(np.uint64) + np.uint64(frames), np.uint64(max_history)).astype(np.uint32)
            count = np.where(kept, total, count).astype(np.uint32)
    rgba = None
    if encode is not None:
        rgba = encode(np.ascontiguousarray(out.reshape(-1, 4)), bool(flags & SRGB_POW)).reshape(h, w)
    return out, count, rgba
