"""rt_reproject_clip's quality on the GPU ("Clamping the carried history"): the 24-move sequence of
tests/reproject_clip_seq.py on the three built-in scenes with the library's own planes -- rt_trace's 1-spp means and
means of frames 1..256, rt_trace_first_hit's Hit plane at the pixel centre -- carried by rt_reproject and by
rt_reproject_clip at the library's defaults and at Radius 2, Gamma 1 (MaxHistory and DepthTolerance the defaults).
Prints, per scene and setting, the MSE over the raw 1-spp MSE as the mean of moves 2..6, 7..12 and 13..24: of the
carried frame, and of the carried frame after rt_denoise's defaults (restated in numpy: tests/denoise_ref.py, which
the GPU's rt_denoise equals bit for bit).  The CPU's figures on the oracle's planes are
profiles/reproject_clip_defaults.txt.

    python scripts/reproject_clip_quality.py > profiles/reproject_clip_quality.txt     (needs the GPU)
"""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

SPANS = ((2, 6), (7, 12), (13, 24))


def spans(ratios):
    return [sum(ratios[a - 1:b]) / (b - a + 1) for a, b in SPANS]


def main():
    import torch

    import __graft_entry__ as graft
    import reproject_clip_seq as cseq
    import reproject_seq as seq
    from test_gpu_reproject import Loop, pack_hit
    rt = graft.load_package()
    d = rt.reproject_clip_defaults()
    stream = torch.cuda.current_stream().cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    def gpu_step(clip):
        def step(mean, key, t, cam, prev, history, hist_key, hist_t, hist_count):
            h, w = key.shape
            keep = [up(mean), up(pack_hit(key, t).view(np.int32)), up(history), up(pack_hit(hist_key, hist_t).view(np.int32)),
                    up(hist_count.view(np.int32))]
            out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            count = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            call, extra = (rt.reproject_clip, dict(radius=clip[0], gamma=clip[1])) if clip else (rt.reproject, {})
            call(w, h, cam, prev, keep[0].data_ptr(), keep[1].data_ptr(), out.data_ptr(), count.data_ptr(),
                 history_ptr=keep[2].data_ptr(), history_hit_ptr=keep[3].data_ptr(), history_count_ptr=keep[4].data_ptr(),
                 max_history=d["max_history"], depth_tolerance=d["depth_tolerance"], stream=stream, **extra)
            torch.cuda.synchronize()
            return out.cpu().numpy(), count.cpu().numpy().view(np.uint32)
        return step

    print(f"# MSE / raw 1-spp MSE, {seq.W}x{seq.H}, {seq.BOUNCES} bounces, {cseq.MOVES} moves, the library's own planes, "
          f"MaxHistory {d['max_history']}, DepthTolerance {d['depth_tolerance']:.3g}; columns: the mean of moves " +
          ", ".join(f"{a}..{b}" for a, b in SPANS) + " of the carried frame | the same after the default rt_denoise")
    settings = [("rt_reproject", None), (f"R {d['radius']} gamma {d['gamma']:.3g} (defaults)", (d["radius"], d["gamma"])),
                ("R 2 gamma 1", (2, 1.0))]
    for name, (index, prefix) in seq.SCENES.items():
        lp = Loop(rt, torch, index, prefix, seq.W, seq.H, max_bounce=seq.BOUNCES)
        try:
            cams, fresh, hits, refs = [], [], [], []
            for i, ang in enumerate(seq.angles(lp.scene.DefaultXAngle, cseq.MOVES)):
                cam = lp.camera(x_angle=float(ang))
                m0 = lp.trace(cam)
                hit = lp.first_hit(cam)
                cams.append(cam)
                fresh.append(m0)
                hits.append((hit[..., 0].copy(), hit[..., 1].view(np.float32).copy()))
                if i:
                    refs.append(seq.mean_without_frame_0(m0, lp.trace(cam, frames=seq.REF_FRAMES, prev_count=1, prev=m0),
                                                         seq.REF_FRAMES))
        finally:
            lp.dev.close()
        print(f"scene {name}")
        floats = [rt.camera_floats(c) for c in cams]
        for label, clip in settings:
            # (cseq.run carries the first frame through the numpy restatement, which wants the camera's floats)
            step = gpu_step(clip)
            by_floats = {id(f): c for f, c in zip(floats, cams)}
            res = cseq.run(floats, fresh, hits, refs,
                           lambda m, k, t, c, p, *hist: step(m, k, t, by_floats[id(c)], by_floats[id(p)], *hist),
                           post=cseq.default_denoise)
            before, after = spans([a / c for a, _, c in res]), spans([b / c for _, b, c in res])
            print(f"  {label:<28} " + " ".join(f"{v:.3f}" for v in before) + "  |  " + " ".join(f"{v:.3f}" for v in after),
                  flush=True)


if __name__ == "__main__":
    main()
