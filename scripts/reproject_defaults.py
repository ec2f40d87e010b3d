"""How rt_reproject_defaults' MaxHistory and DepthTolerance were chosen ("Carrying the mean across a
camera move"): the numpy restatement (tests/reproject_ref.py) over the six-move sequence of tests/reproject_seq.py --
136 x 104, 8 bounces, six orbit steps of 1/16 rad, 1 fresh spp per move, the CPU oracle's means and an f64 first
hit -- on the three built-in scenes, for DepthTolerance in {0, 0.02, 0.05, 0.1, 0.25} and MaxHistory in {8, 16, 32,
64}.  Prints, per scene and setting, the reprojected MSE over the raw 1-spp MSE at each move and the mean of moves
2..6; then, because six moves at 1 spp never reach a cap of 8, the four caps over an orbit of 48 moves at the chosen
tolerance.  CPU only; a few minutes.

    python scripts/reproject_defaults.py > profiles/reproject_defaults.txt
"""
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

TOLERANCES = (0.0, 0.02, 0.05, 0.1, 0.25)
CAPS = (8, 16, 32, 64)
LONG_MOVES, LONG_TOLERANCE, LONG_SHOWN = 48, 0.1, (6, 12, 24, 36, 48)


def main():
    import reproject_seq as seq
    from oracle import oracle as orc
    orc.lib()
    print(f"# reprojected MSE / raw 1-spp MSE, {seq.W}x{seq.H}, {seq.BOUNCES} bounces, against the mean of frames "
          f"1..{seq.REF_FRAMES}; columns: moves 1..{seq.MOVES}, then the mean of moves 2..{seq.MOVES}")
    summary = {}
    for name, (index, prefix) in seq.SCENES.items():
        cams, fresh, hits, refs = seq.oracle_inputs(orc, index, prefix)
        print(f"scene {name}: raw MSE per move " + " ".join(f"{seq.mse(fresh[i + 1], refs[i]):.4e}" for i in range(seq.MOVES)))
        for tol in TOLERANCES:
            for cap in CAPS:
                r = [a / b for a, b in seq.run(cams, fresh, hits, refs, max_history=cap, depth_tolerance=tol)]
                tail = sum(r[1:]) / len(r[1:])
                summary.setdefault((tol, cap), []).append(tail)
                print(f"  tol {tol:<5} cap {cap:<3} " + " ".join(f"{v:.3f}" for v in r) + f"   {tail:.3f}", flush=True)
    print("# mean of moves 2..6 per scene, and over the three scenes")
    for (tol, cap), tails in summary.items():
        print(f"  tol {tol:<5} cap {cap:<3} " + " ".join(f"{v:.3f}" for v in tails) + f"   {sum(tails) / len(tails):.3f}")
    # six moves at 1 spp never reach a cap of 8: the cap is chosen on a longer orbit, at the tolerance chosen above
    print(f"# {LONG_MOVES} moves at tol {LONG_TOLERANCE}: the ratio at moves {', '.join(map(str, LONG_SHOWN))}, then the "
          f"mean of moves {LONG_MOVES // 2 + 1}..{LONG_MOVES}")
    for name, (index, prefix) in seq.SCENES.items():
        cams, fresh, hits, refs = seq.oracle_inputs(orc, index, prefix, moves=LONG_MOVES)
        for cap in CAPS:
            r = [a / b for a, b in seq.run(cams, fresh, hits, refs, max_history=cap, depth_tolerance=LONG_TOLERANCE)]
            tail = r[LONG_MOVES // 2:]
            print(f"  scene {name:<13} cap {cap:<3} " + " ".join(f"{r[m - 1]:.3f}" for m in LONG_SHOWN) +
                  f"   {sum(tail) / len(tail):.3f}", flush=True)


if __name__ == "__main__":
    main()
