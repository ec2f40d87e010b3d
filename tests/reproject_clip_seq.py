"""The 24-move sequence rt_reproject_clip is judged on (not a test): tests/reproject_seq.py's sequence -- 136 x 104, 8
bounces, orbit steps of 1/16 rad, 1 fresh spp per move, the mean of frames 1..256 as the truth -- held for MOVES = 24
moves, since what the clamp removes is the stale reflection that builds up while a key is held.  Shared by
tests/test_reproject_clip_ref.py (the oracle's means), scripts/reproject_clip_defaults.py and
scripts/reproject_clip_quality.py (the library's own planes).

    plain(**settings) / clipped(radius, gamma, **settings)  -> a step function over the numpy restatements
    run(cams, fresh, hits, refs, step, post=None)           -> per move (carried MSE, filtered MSE or None, raw MSE)
    default_denoise(out, key, t)                            -> rt_denoise's defaults restated: the frame a loop shows
    tail(values)                                            -> the mean of moves 13..24
"""
import numpy as np

import reproject_clip_ref as rc
import reproject_ref as rr
import reproject_seq as seq

MOVES = 24
TAIL = slice(12, 24)  # moves 13..24


def plain(**kw):
    return lambda *planes: rr.reproject(*planes, **kw)


def clipped(radius, gamma, **kw):
    return lambda *planes: rc.reproject_clip(*planes, radius=radius, gamma=gamma, **kw)


def default_denoise(out, key, t):
    """rt_denoise_defaults restated (tests/denoise_ref.py): three passes, SigmaDepth 0.25, SigmaColor 0.5, no normal
    stop, not demodulated."""
    import denoise_ref
    return denoise_ref.denoise(out, key, t, iterations=3, sigma_depth=0.25, sigma_color=0.5)[0]


def run(cams, fresh, hits, refs, step, post=None):
    """cams, fresh, hits, refs as tests/reproject_seq.py oracle_inputs gives them.  `step(mean, key, t, cam, prev_cam,
    history, hist_key, hist_t, hist_count)` -> (Out, OutCount, ...); the first frame is carried without history by
    rr.reproject.  `post(out, key, t)`: the filter between the carried frame and the screen (it does not feed the
    history)."""
    hist, cnt, _ = rr.reproject(fresh[0], hits[0][0], hits[0][1], cams[0], cams[0], max_history=1)
    res = []
    for i in range(1, len(cams)):
        hist, cnt = step(fresh[i], hits[i][0], hits[i][1], cams[i], cams[i - 1], hist, hits[i - 1][0], hits[i - 1][1], cnt)[:2]
        shown = None if post is None else seq.mse(post(hist, hits[i][0], hits[i][1]), refs[i - 1])
        res.append((seq.mse(hist, refs[i - 1]), shown, seq.mse(fresh[i], refs[i - 1])))
    return res


def tail(values):
    v = list(values)[TAIL]
    return sum(v) / len(v)
