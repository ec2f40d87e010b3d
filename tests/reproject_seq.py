"""The camera-move sequence rt_reproject is judged on (not a test): shared by tests/test_reproject_ref.py (the
oracle's means on the CPU), tests/test_gpu_reproject.py (the library's own planes) and scripts/reproject_defaults.py.

A 136 x 104 image at 8 bounces; the camera starts at the scene's default orbit and takes MOVES steps of 1/16 rad
(rt_on_render's key step), one fresh sample per pixel after each.  The history starts as the 1-spp frame of the
first camera.  Per move: the reprojected frame and the raw 1-spp frame are compared, as the mean squared error on
channels clamped to [0, 1], with the mean of frames 1..REF_FRAMES at that camera (the fresh sample is frame 0 and
is not in it).

    angles(x_angle, moves)                -> the moves + 1 orbit angles, accumulated in f32 as rt_on_render does
    mean_without_frame_0(m0, m_all, n)    -> mean of frames 1..n from frame 0 alone and the mean of frames 0..n
    hit_planes_f64(camf, spheres, w, h)   -> (key (H, W) u32, t (H, W) f32): an f64 first hit at the pixel centre
    run(frames, reproject, ...)           -> per move (reprojected MSE, raw MSE)
"""
import numpy as np

import reproject_ref as rr

W, H, BOUNCES, MOVES, REF_FRAMES = 136, 104, 8, 6, 256
STEP = np.float32(1.0 / 16.0)
SCENES = {"0 RGB Glass": (0, None), "1 prefix 64": (1, 64), "2 RTWeekend": (2, None)}


def angles(x_angle, moves=MOVES):
    out = [np.float32(x_angle)]
    for _ in range(moves):
        out.append(np.float32(out[-1] + STEP))
    return out


def mean_without_frame_0(frame0, mean_0_to_n, n):
    """(H, W, 4) f64: ((n + 1) * mean of frames 0..n - frame 0) / n."""
    return ((n + 1) * mean_0_to_n.astype(np.float64) - frame0.astype(np.float64)) / n


def mse(a, ref):
    return float(((np.clip(a[..., :3].astype(np.float64), 0, 1) - np.clip(ref[..., :3], 0, 1)) ** 2).mean())


def hit_planes_f64(camf, spheres, w, h):
    """Key = the nearest sphere's index, RT_HIT_INSIDE where the ray starts inside it, RT_HIT_MISS on a miss; T its
    distance rounded to f32, 1e30f on a miss (tests/test_gpu_first_hit.py first_hit_f64, the pixel centre)."""
    from test_gpu_first_hit import first_hit_f64
    f = first_hit_f64(np.asarray(camf, np.float32), spheres, w, h)
    miss = f["win"] < 0
    key = np.where(miss, rr.HIT_MISS, f["win"].astype(np.uint32) | np.where(f["inside"], rr.HIT_INSIDE, np.uint32(0)))
    t = np.where(miss, np.float32(1e30), f["t"].astype(np.float32))
    return key.astype(np.uint32).reshape(h, w), t.astype(np.float32).reshape(h, w)


def run(cams, fresh, hits, refs, *, max_history, depth_tolerance, reproject=None):
    """cams, fresh, hits: MOVES + 1 cameras (24 floats), 1-spp means (H, W, 4) and (key, t) pairs; refs: MOVES
    reference means for cameras 1...  `reproject`: a function with rr.reproject's signature (default: rr.reproject
    itself; the GPU test passes the library's).  Returns [(reprojected MSE, raw MSE)] per move."""
    reproject = reproject or rr.reproject
    hist, cnt, _ = reproject(fresh[0], hits[0][0], hits[0][1], cams[0], cams[0], max_history=max_history,
                             depth_tolerance=depth_tolerance)
    assert np.array_equal(hist.view(np.uint32), fresh[0].view(np.uint32)) and (cnt == 1).all()
    out = []
    for i in range(1, len(cams)):
        hist, cnt, _ = reproject(fresh[i], hits[i][0], hits[i][1], cams[i], cams[i - 1], hist, hits[i - 1][0],
                                 hits[i - 1][1], cnt, max_history=max_history, depth_tolerance=depth_tolerance)
        out.append((mse(hist, refs[i - 1]), mse(fresh[i], refs[i - 1])))
    return out


def oracle_inputs(orc, scene_index, prefix, threads=None, moves=MOVES):
    """(cams, fresh, hits, refs) of one built-in scene from the CPU oracle and the f64 first hit."""
    sc = orc.scene_builtin(scene_index)
    if prefix:
        sc = sc.prefix(prefix)
    threads = threads or orc.cpu_threads()
    cams, fresh, hits, refs = [], [], [], []
    for i, ang in enumerate(angles(sc.x_angle, moves)):
        cam = orc.camera(sc, W, H, x_angle=float(ang))
        m0, _, _ = orc.render(sc, cam, W, H, frames=1, max_bounce=BOUNCES, threads=threads)
        cams.append(cam)
        fresh.append(m0.reshape(H, W, 4).copy())
        hits.append(hit_planes_f64(cam, sc.spheres, W, H))
        if i:
            m, _, _ = orc.render(sc, cam, W, H, prev_count=1, frames=REF_FRAMES, max_bounce=BOUNCES, threads=threads,
                                 prev=m0.copy())
            refs.append(mean_without_frame_0(fresh[-1], m.reshape(H, W, 4), REF_FRAMES))
    return cams, fresh, hits, refs
