"""Generates tests/golden/random_scene_digests.json: one sha256 per seed 0..55 of everything
tests/random_scenes.make(seed) produces -- the sphere records' bytes, the sky flag and every
camera's floats and kind.  tests/test_random_scene_inputs.py checks that the generator still
gives these digests, so that seeded scenes keep every byte while the generator grows overrides.
Written once, from the generator as it stood before it had any override; run it again only
where a change of the seeded scenes is intended.

    python tests/golden/make_random_scene_digests.py
"""
import hashlib
import json
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
import random_scenes  # noqa: E402

OUT = pathlib.Path(__file__).with_name("random_scene_digests.json")
SEEDS = range(56)


def digest(spec) -> str:
    """sha256 over spheres.tobytes(), use_sky and each camera's floats (as f64) and kind."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(spec["spheres"], np.float32).tobytes())
    h.update(b"\x01" if spec["use_sky"] else b"\x00")
    for look, dist, ang, yh, kind in spec["cameras"]:
        h.update(np.array([*look, dist, ang, yh], np.float64).tobytes())
        h.update(kind.encode())
    return h.hexdigest()


def main():
    out = {"generator": "tests/golden/make_random_scene_digests.py",
           "digest": "sha256(spheres f32 bytes, use_sky byte, per camera: look_at[3] distance x_angle y_height as f64, kind)",
           "seeds": {str(s): digest(random_scenes.make(s)) for s in SEEDS}}
    OUT.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
