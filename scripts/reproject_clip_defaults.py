"""How rt_reproject_clip_defaults' Radius and Gamma were chosen ("Clamping the carried history"): the
numpy restatements (tests/reproject_clip_ref.py, tests/reproject_ref.py) over the 24-move sequence of
tests/reproject_clip_seq.py -- 136 x 104, 8 bounces, 24 orbit steps of 1/16 rad, 1 fresh spp per move, the CPU
oracle's means and an f64 first hit -- on the three built-in scenes, for Radius in {1, 2, 3} x Gamma in {0.5, 1, 2}
at MaxHistory 8 and 32 (DepthTolerance 0.1), beside plain rt_reproject at the same caps.  Every figure is an MSE over
the raw 1-spp MSE of the same move, averaged over moves 2..6, 7..12 and 13..24: of the carried frame, and of the
carried frame after rt_denoise's defaults restated (three passes, SigmaDepth 0.25, SigmaColor 0.5, no normal stop),
which is what a loop shows.  The setting with the lowest three-scene mean of moves 13..24 after the filter is the
default; ties go to the smaller radius.  CPU only; a quarter of an hour.

    python scripts/reproject_clip_defaults.py > profiles/reproject_clip_defaults.txt
"""
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

RADII, GAMMAS, CAPS, TOLERANCE = (1, 2, 3), (0.5, 1.0, 2.0), (8, 32), 0.1
SPANS = ((2, 6), (7, 12), (13, 24))


def spans(ratios):
    return [sum(ratios[a - 1:b]) / (b - a + 1) for a, b in SPANS]


def main():
    import reproject_clip_seq as cseq
    import reproject_seq as seq
    from oracle import oracle as orc
    orc.lib()
    print(f"# MSE / raw 1-spp MSE, {seq.W}x{seq.H}, {seq.BOUNCES} bounces, {cseq.MOVES} moves, against the mean of frames "
          f"1..{seq.REF_FRAMES}, DepthTolerance {TOLERANCE}; columns: the mean of moves " +
          ", ".join(f"{a}..{b}" for a, b in SPANS) + " of the carried frame | the same after the default rt_denoise")
    table = {}
    for name, (index, prefix) in seq.SCENES.items():
        cams, fresh, hits, refs = seq.oracle_inputs(orc, index, prefix, moves=cseq.MOVES)
        print(f"scene {name}")
        for cap in CAPS:
            kw = dict(max_history=cap, depth_tolerance=TOLERANCE)
            settings = [("rt_reproject", None, None, cseq.plain(**kw))]
            settings += [(f"R {r} gamma {g:<3}", r, g, cseq.clipped(r, g, **kw)) for r in RADII for g in GAMMAS]
            for label, r, g, step in settings:
                res = cseq.run(cams, fresh, hits, refs, step, post=cseq.default_denoise)
                before, after = spans([a / c for a, _, c in res]), spans([b / c for _, b, c in res])
                table.setdefault((cap, label, r, g), []).append((before[-1], after[-1]))
                print(f"  cap {cap:<2} {label:<14} " + " ".join(f"{v:.3f}" for v in before) + "  |  " +
                      " ".join(f"{v:.3f}" for v in after), flush=True)
    print("# moves 13..24 per scene (0, 1 prefix 64, 2) and their mean: carried | after the default rt_denoise")
    best = None
    for (cap, label, r, g), rows in table.items():
        b, a = [x for x, _ in rows], [y for _, y in rows]
        mb, ma = sum(b) / len(b), sum(a) / len(a)
        print(f"  cap {cap:<2} {label:<14} " + " ".join(f"{v:.3f}" for v in b) + f"  {mb:.3f}  |  " +
              " ".join(f"{v:.3f}" for v in a) + f"  {ma:.3f}")
        if r is not None and (best is None or (round(ma, 3), r) < best[0]):
            best = ((round(ma, 3), r), cap, label)
    print(f"# lowest three-scene mean of moves 13..24 after the filter (ties to three decimals: the smaller radius): "
          f"cap {best[1]}, {best[2]}: {best[0][0]:.3f}")


if __name__ == "__main__":
    main()
